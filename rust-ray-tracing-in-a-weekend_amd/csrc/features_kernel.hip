// features_kernel.hip — host-side dispatch of rt_render_features' trace_features variants
// (features_v_*.hip over features_device.hpp) and the reduction of their chunk partials.
#include "features_device.hpp"

namespace rtk {

// reduce_chunks over the seven feature channels: per pixel the partials added in chunk order to
// 0.0 (or, from the second buffer batch on, to the running sums in acc: the same additions in the
// same order as one launch), then sum * scale into the frames the caller asked for.
__global__ void __launch_bounds__(256) reduce_features(const double* __restrict__ partial, double* __restrict__ acc,
                                                       double* __restrict__ albedo, double* __restrict__ normal,
                                                       double* __restrict__ depth, long long n_px, int n_chunks,
                                                       int first, int last, double scale)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_px) return;
    double v[kFeatureChannels];
#pragma unroll
    for (int j = 0; j < kFeatureChannels; ++j) v[j] = first ? 0.0 : acc[(size_t)i * kFeatureChannels + j];
    for (int c = 0; c < n_chunks; ++c) {
        const double* p = partial + ((size_t)c * n_px + i) * kFeatureChannels;
#pragma unroll
        for (int j = 0; j < kFeatureChannels; ++j) v[j] = v[j] + p[j];
    }
    if (!last) {
#pragma unroll
        for (int j = 0; j < kFeatureChannels; ++j) acc[(size_t)i * kFeatureChannels + j] = v[j];
        return;
    }
    if (albedo) {
        albedo[3 * i + 0] = v[0] * scale;
        albedo[3 * i + 1] = v[1] * scale;
        albedo[3 * i + 2] = v[2] * scale;
    }
    if (normal) {
        normal[3 * i + 0] = v[3] * scale;
        normal[3 * i + 1] = v[4] * scale;
        normal[3 * i + 2] = v[5] * scale;
    }
    if (depth) depth[i] = v[6] * scale;
}

hipError_t launch_features(const SceneDev& S, const KParams& Ph, const KParams* P, double* partial,
                           const LaunchOpts& o, hipStream_t stream)
{
    if (o.f32 || o.count) return hipErrorNotSupported;
    Launch L;
    L.S = &S;
    L.P = P;
    L.out = partial;
    L.counters = nullptr;
    L.work = nullptr;
    L.pool = 0;
    L.waves_per_simd = o.waves_per_simd;
    L.n_blocks = (unsigned long long)Ph.tiles_x * Ph.tiles_y * Ph.n_chunks;   // waves: one per (tile, chunk)
    if (L.n_blocks == 0) return hipSuccess;
    if (L.n_blocks > 0xfffffff0ULL) return hipErrorInvalidValue;
    const uint32_t f = variant_features(o.features);
    if (f == FEAT_SET_SPHERES) return launch_features_variant<FEAT_SET_SPHERES>(L, o, stream);
    if (f == FEAT_SET_RECTINST) return launch_features_variant<FEAT_SET_RECTINST>(L, o, stream);
    if (f == FEAT_SET_MEDIA) return launch_features_variant<FEAT_SET_MEDIA>(L, o, stream);
    if (f == FEAT_SET_FINAL) return launch_features_variant<FEAT_SET_FINAL>(L, o, stream);
    return launch_features_variant<FEAT_ALL>(L, o, stream);
}

hipError_t launch_reduce_features(const double* partial, double* acc, double* albedo, double* normal, double* depth,
                                  long long n_px, int n_chunks, bool first, bool last, double scale,
                                  hipStream_t stream)
{
    const long long blocks = (n_px + 255) / 256;
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reduce_features, dim3((unsigned)blocks), dim3(256), 0, stream, partial, acc, albedo, normal, depth,
                       n_px, n_chunks, (int)first, (int)last, scale);
    return hipGetLastError();
}

}  // namespace rtk
