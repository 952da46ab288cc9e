// pyramid_kernel.hip — the device half of rt_denoise_pyramid (include/rt/rt_abi.h): the NL-means
// filter of denoise_kernel.hip run at several scales of a mean frame, its standard-error map and
// optional first-hit guides, the coarse scales supplying the low frequencies the fine window cannot
// see. The arithmetic around the filter is pyramid_core.hpp's, shared with the host filter
// (pyramid_host.cpp); the filter itself is launch_denoise, unchanged, on f64 frames.
//
// A call of L >= 2 levels enqueues, in order:
//   pyramid_widen    (f32 input only) C_0 = the frame as f64
//   pyramid_down     l = 0..L-2: C_{l+1}, s_{l+1} and every guide present, one launch per level
//   launch_denoise   l = 0..L-1: D_l, f64; the levels above 0 on a second stream beside level 0
//                    (PyramidSide: forked after Down, joined before Up)
//   pyramid_diff     l = L-2..0: K_l = R_{l+1} - the block mean of D_l, on the coarse grid
//   pyramid_up_add   l = L-2..0: R_l = D_l + the four-tap correction from K_l; in place over D_l,
//                    except at level 0, which writes out in the caller's format behind the
//                    keep-the-input rule
// These are streaming kernels: one thread per output pixel in raster order, 256-thread workgroups,
// so a wave reads and writes consecutive pixels of a row (a Down or diff thread reads two adjacent
// fine pixels per row, 48 consecutive bytes of a colour frame). No LDS, no atomics, no
// cross-workgroup state: a pixel's value depends on the frames alone, so the result repeats bit for
// bit. Every read is behind its pixel's inside-the-frame test (pyramid_core.hpp: blocks are cut at
// the frame's edge, tap coordinates are clamped).
#include "denoise.hpp"
#include "pyramid.hpp"
#include "pyramid_core.hpp"

namespace rtk {

constexpr int kPyramidThreads = 256;

__global__ void __launch_bounds__(kPyramidThreads)
    pyramid_widen(const float* __restrict__ M, double* __restrict__ C, size_t hw)
{
    const size_t i = (size_t)blockIdx.x * kPyramidThreads + threadIdx.x;
    if (i >= hw) return;
    C[3 * i + 0] = (double)M[3 * i + 0];
    C[3 * i + 1] = (double)M[3 * i + 1];
    C[3 * i + 2] = (double)M[3 * i + 2];
}

// the fine frames of a level and the coarse frames Down writes (a guide not given: both null)
struct PyramidDownFrames {
    const double* c;
    const double* s;
    const double* a;
    const double* n;
    const double* z;
    double* c_out;
    double* s_out;
    double* a_out;
    double* n_out;
    double* z_out;
};

__global__ void __launch_bounds__(kPyramidThreads) pyramid_down(PyramidDownFrames f, int W, int H, int wc, int hc)
{
    const size_t i = (size_t)blockIdx.x * kPyramidThreads + threadIdx.x;
    if (i >= (size_t)wc * (size_t)hc) return;
    const int cy = (int)(i / (size_t)wc), cx = (int)(i - (size_t)cy * (size_t)wc);
    for (int ch = 0; ch < 3; ++ch) f.c_out[3 * i + ch] = pyramid_block_mean(f.c, 3, ch, W, H, cx, cy);
    f.s_out[i] = pyramid_block_se(f.s, W, H, cx, cy);
    if (f.a)
        for (int ch = 0; ch < 3; ++ch) f.a_out[3 * i + ch] = pyramid_block_mean(f.a, 3, ch, W, H, cx, cy);
    if (f.n)
        for (int ch = 0; ch < 3; ++ch) f.n_out[3 * i + ch] = pyramid_block_mean(f.n, 3, ch, W, H, cx, cy);
    if (f.z) f.z_out[i] = pyramid_block_mean(f.z, 1, 0, W, H, cx, cy);
}

// K(c) = R_coarse(c) - the block mean of D over c's block; D is W x H, R_coarse and K are wc x hc
__global__ void __launch_bounds__(kPyramidThreads)
    pyramid_diff(const double* __restrict__ D, const double* __restrict__ Rc, double* __restrict__ K, int W, int H, int wc,
                 int hc)
{
    const size_t i = (size_t)blockIdx.x * kPyramidThreads + threadIdx.x;
    if (i >= (size_t)wc * (size_t)hc) return;
    const int cy = (int)(i / (size_t)wc), cx = (int)(i - (size_t)cy * (size_t)wc);
    for (int ch = 0; ch < 3; ++ch) K[3 * i + ch] = Rc[3 * i + ch] - pyramid_block_mean(D, 3, ch, W, H, cx, cy);
}

// R(p) = D(p) + u(p). FINAL: R is the call's out in format T, and a pixel whose Y(M) or se is not
// finite keeps M; otherwise T is double and R may be D itself (a thread reads and writes its own
// pixel only).
template <bool FINAL, typename T>
__global__ void __launch_bounds__(kPyramidThreads)
    pyramid_up_add(const double* D, const double* __restrict__ K, T* R, const T* __restrict__ M,
                   const double* __restrict__ se, int W, int H, int wc, int hc)
{
    const size_t i = (size_t)blockIdx.x * kPyramidThreads + threadIdx.x;
    if (i >= (size_t)W * (size_t)H) return;
    const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * (size_t)W);
    double u[3];
    pyramid_correction(K, wc, hc, x, y, u);
    const double r0 = D[3 * i + 0] + u[0], r1 = D[3 * i + 1] + u[1], r2 = D[3 * i + 2] + u[2];
    if constexpr (FINAL) {
        const T m0 = M[3 * i + 0], m1 = M[3 * i + 1], m2 = M[3 * i + 2];
        const bool keep = !denoise_finite(denoise_luma((double)m0, (double)m1, (double)m2)) || !denoise_finite(se[i]);
        R[3 * i + 0] = keep ? m0 : (T)r0;
        R[3 * i + 1] = keep ? m1 : (T)r1;
        R[3 * i + 2] = keep ? m2 : (T)r2;
    } else {
        R[3 * i + 0] = r0;
        R[3 * i + 1] = r1;
        R[3 * i + 2] = r2;
    }
}

namespace {

// workgroups of one thread per pixel; 0 if they do not fit a launch
unsigned pyramid_blocks(size_t pixels)
{
    const size_t b = (pixels + kPyramidThreads - 1) / kPyramidThreads;
    return b > 0x7fffffffULL ? 0u : (unsigned)b;
}

template <typename T>
hipError_t launch_final(const double* D, const double* K, void* out, const void* mean, const double* se, int W, int H,
                        int wc, int hc, hipStream_t stream)
{
    hipLaunchKernelGGL((pyramid_up_add<true, T>), dim3(pyramid_blocks((size_t)W * (size_t)H)), dim3(kPyramidThreads), 0,
                       stream, D, K, (T*)out, (const T*)mean, se, W, H, wc, hc);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pyramid(const void* mean, const double* se, void* out, bool f64, int width, int height, int radius,
                          int patch, double k, int levels, const DenoiseGuides& guides, double* scratch,
                          hipStream_t stream, const PyramidSide& side)
{
    if (width < 1 || height < 1 || levels < 1 || levels > kPyramidMaxLevels) return hipErrorInvalidValue;
    if (levels == 1) return launch_denoise(mean, se, out, f64, width, height, radius, patch, k, guides, stream);
    if (!scratch || !pyramid_blocks((size_t)width * (size_t)height)) return hipErrorInvalidValue;
    const PyramidLayout lay(width, height, levels, f64, guides.albedo != nullptr, guides.normal != nullptr,
                            guides.depth != nullptr);

    // a level's frames: the caller's at level 0, the scratch's above
    const double* C[kPyramidMaxLevels];
    const double* S[kPyramidMaxLevels];
    DenoiseGuides G[kPyramidMaxLevels];
    C[0] = f64 ? (const double*)mean : scratch + lay.c[0];
    S[0] = se;
    G[0] = guides;
    for (int l = 1; l < levels; ++l) {
        C[l] = scratch + lay.c[l];
        S[l] = scratch + lay.s[l];
        G[l] = guides;   // (the sigmas are every level's)
        if (guides.albedo) G[l].albedo = scratch + lay.a[l];
        if (guides.normal) G[l].normal = scratch + lay.n[l];
        if (guides.depth) G[l].depth = scratch + lay.z[l];
    }
    auto D = [&](int l) { return scratch + lay.d[l]; };
    double* const K = scratch + lay.k;

    if (!f64) {
        const size_t hw = (size_t)width * (size_t)height;
        hipLaunchKernelGGL(pyramid_widen, dim3(pyramid_blocks(hw)), dim3(kPyramidThreads), 0, stream, (const float*)mean,
                           scratch + lay.c[0], hw);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    for (int l = 0; l + 1 < levels; ++l) {
        const PyramidDownFrames f{C[l],
                                  S[l],
                                  G[l].albedo,
                                  G[l].normal,
                                  G[l].depth,
                                  scratch + lay.c[l + 1],
                                  scratch + lay.s[l + 1],
                                  guides.albedo ? scratch + lay.a[l + 1] : nullptr,
                                  guides.normal ? scratch + lay.n[l + 1] : nullptr,
                                  guides.depth ? scratch + lay.z[l + 1] : nullptr};
        hipLaunchKernelGGL(pyramid_down, dim3(pyramid_blocks((size_t)lay.w[l + 1] * (size_t)lay.h[l + 1])),
                           dim3(kPyramidThreads), 0, stream, f, lay.w[l], lay.h[l], lay.w[l + 1], lay.h[l + 1]);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    // the levels' filters are independent: the coarse ones on the side stream, between fork and join
    hipStream_t coarse = side.side ? side.side : stream;
    if (side.side) {
        if (hipError_t e = hipEventRecord(side.fork, stream); e != hipSuccess) return e;
        if (hipError_t e = hipStreamWaitEvent(side.side, side.fork, 0); e != hipSuccess) return e;
    }
    // Level 0 first, then the others from the coarsest: the smallest levels are under a workgroup
    // per CU and cost a workgroup's latency each, which passes beside level 0; level 1, the only
    // other one with work to speak of, then shares the device with the rest of level 0.
    hipError_t err = launch_denoise(C[0], S[0], D(0), true, lay.w[0], lay.h[0], radius, patch, k, G[0], stream);
    for (int l = levels - 1; l >= 1 && err == hipSuccess; --l)
        err = launch_denoise(C[l], S[l], D(l), true, lay.w[l], lay.h[l], radius, patch, k, G[l], coarse);
    if (side.side) {   // joined on every way out: what the side stream got must be over when the call's stream is
        hipError_t e = hipEventRecord(side.join, side.side);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, side.join, 0);
        if (err == hipSuccess) err = e;
    }
    if (err != hipSuccess) return err;
    for (int l = levels - 2; l >= 0; --l) {
        const int W = lay.w[l], H = lay.h[l], wc = lay.w[l + 1], hc = lay.h[l + 1];
        hipLaunchKernelGGL(pyramid_diff, dim3(pyramid_blocks((size_t)wc * (size_t)hc)), dim3(kPyramidThreads), 0, stream,
                           (const double*)D(l), (const double*)D(l + 1), K, W, H, wc, hc);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        if (l > 0) {
            hipLaunchKernelGGL((pyramid_up_add<false, double>), dim3(pyramid_blocks((size_t)W * (size_t)H)),
                               dim3(kPyramidThreads), 0, stream, (const double*)D(l), (const double*)K, D(l),
                               (const double*)nullptr, (const double*)nullptr, W, H, wc, hc);
            if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        } else {
            const hipError_t e = f64 ? launch_final<double>(D(0), K, out, mean, se, W, H, wc, hc, stream)
                                     : launch_final<float>(D(0), K, out, mean, se, W, H, wc, hc, stream);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace rtk
