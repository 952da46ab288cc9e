// denoise_kernel.hip — the device half of rt_denoise (include/rt/rt_abi.h): non-local means with
// variance-normalised patch distances over a mean frame and its standard-error map. The
// arithmetic is denoise_core.hpp's, shared with the host filter (denoise_host.cpp).
//
// One 256-thread workgroup filters one 16x16 tile of the frame, thread (lx, ly) its pixel p.
//   1. Y and V = se^2 of the tile and its halo of radius + patch pixels are staged once into LDS
//      as f64 ((16 + 2 (r + f))^2 cells, 28 KB at r = 10, f = 3); a cell outside the image holds
//      V = -1, which no pixel has (se^2 >= 0 or NaN).
//   2. Per offset o, in raster order: the workgroup writes delta(a, o) for the (16 + 2f)^2 cells a
//      its patches cover into one of two LDS planes (0 where a or a + o is outside the image),
//      one barrier, then every thread sums its own (2f + 1)^2 patch directly, row by row, divides
//      by the number of valid terms (closed form, denoise_axis_count), takes the weight and adds
//      w M(p + o), read from global memory, to its four accumulators. The planes alternate, so the
//      next offset's writes need no second barrier: a thread that writes plane i again has passed
//      the barrier after the other plane's writes, which every thread reaches only after its reads
//      of plane i.
// A plane row is 16 (f = 0) or 48 doubles apart: the 32 lanes an LDS read serves together are two
// rows of 16 pixels, and a row stride of 16 mod 32 doubles puts them on all 64 banks once.
// No atomics and no cross-workgroup state: a pixel's sums depend on the frame alone, in raster
// offset order, whatever the tiling, so the result repeats bit for bit.
//
// rt_denoise_guided is the same kernel with G set: the weight takes denoise_core.hpp's feature
// term Phi(p, o) as well, from the guide frames' values at p and at q = p + o, read from global
// memory beside M(q) (frame-sized f64 arrays, L2-resident at these sizes; nothing more in LDS).
// The instantiation without guides holds none of it.
#include "denoise.hpp"
#include "denoise_core.hpp"

namespace rtk {

constexpr int kDenoiseTile = 16;

__host__ __device__ constexpr int denoise_plane_stride(int patch) { return patch == 0 ? 16 : 48; }

template <typename T, int F, bool G>
__global__ void __launch_bounds__(kDenoiseTile * kDenoiseTile) denoise_nlm(const T* __restrict__ M,
                                                                          const double* __restrict__ se,
                                                                          T* __restrict__ out, int W, int H, int tiles_x,
                                                                          int r, double k2, DenoiseGuides guides)
{
    extern __shared__ double lds[];
    constexpr int kThreads = kDenoiseTile * kDenoiseTile;
    constexpr int PW = kDenoiseTile + 2 * F, PS = denoise_plane_stride(F);
    const int h = r + F, SW = kDenoiseTile + 2 * h;
    double* const sY = lds;
    double* const sV = sY + SW * SW;
    double* const planes = sV + SW * SW;   // 2 x PW rows of PS
    const int tid = (int)threadIdx.x, lx = tid & (kDenoiseTile - 1), ly = tid / kDenoiseTile;
    const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * kDenoiseTile;
    const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * kDenoiseTile;

    for (int i = tid; i < SW * SW; i += kThreads) {
        const int cy = i / SW, cx = i - cy * SW;
        const int x = tx0 - h + cx, y = ty0 - h + cy;
        double yv = 0.0, vv = -1.0;
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t a = (size_t)y * (size_t)W + (size_t)x;
            yv = denoise_luma((double)M[3 * a + 0], (double)M[3 * a + 1], (double)M[3 * a + 2]);
            const double s = se[a];
            vv = s * s;
        }
        sY[i] = yv;
        sV[i] = vv;
    }
    __syncthreads();

    const int px = tx0 + lx, py = ty0 + ly;
    const bool inside = px < W && py < H;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, dn = 0.0;
    int it = 0;
    for (int dy = -r; dy <= r; ++dy) {
        const int qy = py + dy;
        const int cnt_y = denoise_axis_count(py, dy, F, H);
        for (int dx = -r; dx <= r; ++dx, ++it) {
            double* const pl = planes + (it & 1) * (PW * PS);
            const bool centre = dx == 0 && dy == 0;
            if (!centre) {
                for (int i = tid; i < PW * PW; i += kThreads) {
                    const int cy = i / PW, cx = i - cy * PW;
                    const int ia = (cy + r) * SW + cx + r, ib = ia + dy * SW + dx;
                    const double va = sV[ia], vb = sV[ib];
                    double d = 0.0;
                    if (!(va < 0.0) && !(vb < 0.0)) d = denoise_delta(sY[ia], va, sY[ib], vb, k2);
                    pl[cy * PS + cx] = d;
                }
            }
            __syncthreads();
            const int qx = px + dx;
            if (!inside || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            double w = 1.0;
            if (!centre) {
                double s = 0.0;
#pragma unroll
                for (int sy = 0; sy <= 2 * F; ++sy) {
#pragma unroll
                    for (int sx = 0; sx <= 2 * F; ++sx) s = s + pl[(ly + sy) * PS + lx + sx];
                }
                const double D = s / (double)(denoise_axis_count(px, dx, F, W) * cnt_y);
                if constexpr (G)
                    w = denoise_weight_guided(D, denoise_phi(guides, (size_t)py * (size_t)W + (size_t)px,
                                                             (size_t)qy * (size_t)W + (size_t)qx));
                else
                    w = denoise_weight(D);
            }
            if (w == 0.0) continue;
            const size_t b = (size_t)qy * (size_t)W + (size_t)qx;
            n0 = n0 + w * (double)M[3 * b + 0];
            n1 = n1 + w * (double)M[3 * b + 1];
            n2 = n2 + w * (double)M[3 * b + 2];
            dn = dn + w;
        }
    }
    if (!inside) return;
    const int ic = (ly + h) * SW + lx + h;
    const size_t a = (size_t)py * (size_t)W + (size_t)px;
    if (!denoise_finite(sY[ic]) || !denoise_finite(sV[ic])) {
        out[3 * a + 0] = M[3 * a + 0];
        out[3 * a + 1] = M[3 * a + 1];
        out[3 * a + 2] = M[3 * a + 2];
        return;
    }
    out[3 * a + 0] = (T)(n0 / dn);
    out[3 * a + 1] = (T)(n1 / dn);
    out[3 * a + 2] = (T)(n2 / dn);
}

int denoise_lds_bytes(int radius, int patch)
{
    const int sw = kDenoiseTile + 2 * (radius + patch), pw = kDenoiseTile + 2 * patch;
    return (2 * sw * sw + 2 * pw * denoise_plane_stride(patch)) * (int)sizeof(double);
}

template <typename T, int F, bool G>
static hipError_t launch_one(const void* mean, const double* se, void* out, int width, int height, int radius,
                             double k, const DenoiseGuides& guides, hipStream_t stream)
{
    const int tiles_x = (width + kDenoiseTile - 1) / kDenoiseTile, tiles_y = (height + kDenoiseTile - 1) / kDenoiseTile;
    const long long tiles = (long long)tiles_x * tiles_y;
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((denoise_nlm<T, F, G>), dim3((unsigned)tiles), dim3(kDenoiseTile * kDenoiseTile),
                       (size_t)denoise_lds_bytes(radius, F), stream, (const T*)mean, se, (T*)out, width, height, tiles_x,
                       radius, k * k, guides);
    return hipGetLastError();
}

template <typename T, bool G>
static hipError_t launch_patch(const void* mean, const double* se, void* out, int width, int height, int radius,
                               int patch, double k, const DenoiseGuides& guides, hipStream_t stream)
{
    switch (patch) {
    case 0: return launch_one<T, 0, G>(mean, se, out, width, height, radius, k, guides, stream);
    case 1: return launch_one<T, 1, G>(mean, se, out, width, height, radius, k, guides, stream);
    case 2: return launch_one<T, 2, G>(mean, se, out, width, height, radius, k, guides, stream);
    case 3: return launch_one<T, 3, G>(mean, se, out, width, height, radius, k, guides, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_denoise(const void* mean, const double* se, void* out, bool f64, int width, int height, int radius,
                          int patch, double k, const DenoiseGuides& guides, hipStream_t stream)
{
    if (width < 1 || height < 1 || radius < 1 || radius > kDenoiseMaxRadius || patch < 0 || patch > kDenoiseMaxPatch)
        return hipErrorInvalidValue;
    if (guides.any())
        return f64 ? launch_patch<double, true>(mean, se, out, width, height, radius, patch, k, guides, stream)
                   : launch_patch<float, true>(mean, se, out, width, height, radius, patch, k, guides, stream);
    return f64 ? launch_patch<double, false>(mean, se, out, width, height, radius, patch, k, guides, stream)
               : launch_patch<float, false>(mean, se, out, width, height, radius, patch, k, guides, stream);
}

}  // namespace rtk
