// cross_kernel.hip — the device half of rt_denoise_cross (include/rt/rt_abi.h): NL-means over two
// half frames, each half filtered with the weights taken from the other, and the error map read off
// their difference. The arithmetic is denoise_core.hpp's and cross_core.hpp's, shared with the host
// filter (cross_host.cpp).
//
// cross_nlm is denoise_nlm's organisation (denoise_kernel.hip) with both halves per offset. One
// 256-thread workgroup filters one 16x16 tile, thread (lx, ly) its pixel p.
//   1. Y_A, Y_B and V = scale se^2 of the tile and its halo of radius + patch pixels are staged once
//      into LDS as f64 (3 (16 + 2 (r + f))^2 cells, 41 KB at r = 10, f = 3); a cell outside the image
//      holds V = -1, which no pixel has; a bad pixel's cell holds NaN for both Y (cross_cell).
//   2. Per offset o, in raster order: the workgroup writes delta_A(a, o) and delta_B(a, o) for the
//      (16 + 2f)^2 cells a its patches cover into one of two pairs of LDS planes (0 where a or a + o
//      is outside the image: the pair test is made once for both halves), one barrier, then every
//      thread sums its own two (2f + 1)^2 patches directly, row by row, divides both by the one
//      number of valid terms, takes the feature term once and the two weights, and adds w_B M_A(p + o)
//      and w_A M_B(p + o), read from global memory, to its eight accumulators. The plane pairs
//      alternate, so the next offset's writes need no second barrier (denoise_kernel.hip says why).
// LDS: (3 SW^2 + 4 PW PS) 8 bytes, 76,128 at (10, 3): two workgroups per CU.
// With an e buffer the kernel also writes e(p) = 0.5 (Y(F_A) - Y(F_B)); cross_stderr_map then takes
// the 3 x 3 rule over it, one thread per pixel. No atomics and no cross-workgroup state: a pixel's
// sums depend on the frames alone, in raster offset order, whatever the tiling.
#include "cross.hpp"
#include "cross_core.hpp"

namespace rtk {

constexpr int kCrossTile = 16;

__host__ __device__ constexpr int cross_plane_stride(int patch) { return patch == 0 ? 16 : 48; }

template <typename T, int F, bool G>
__global__ void __launch_bounds__(kCrossTile * kCrossTile) cross_nlm(const T* __restrict__ MA, const T* __restrict__ MB,
                                                                      const double* __restrict__ se,
                                                                      T* __restrict__ out, double* __restrict__ e_out,
                                                                      int W, int H, int tiles_x, int r, double k2,
                                                                      double scale, DenoiseGuides guides)
{
    extern __shared__ double lds[];
    constexpr int kThreads = kCrossTile * kCrossTile;
    constexpr int PW = kCrossTile + 2 * F, PS = cross_plane_stride(F);
    const int h = r + F, SW = kCrossTile + 2 * h;
    double* const sYa = lds;
    double* const sYb = sYa + SW * SW;
    double* const sV = sYb + SW * SW;
    double* const planes = sV + SW * SW;   // 2 x (A, B) x PW rows of PS
    const int tid = (int)threadIdx.x, lx = tid & (kCrossTile - 1), ly = tid / kCrossTile;
    const int tx0 = (int)(blockIdx.x % (unsigned)tiles_x) * kCrossTile;
    const int ty0 = (int)(blockIdx.x / (unsigned)tiles_x) * kCrossTile;

    for (int i = tid; i < SW * SW; i += kThreads) {
        const int cy = i / SW, cx = i - cy * SW;
        const int x = tx0 - h + cx, y = ty0 - h + cy;
        CrossCell c{0.0, 0.0, -1.0};
        if (x >= 0 && x < W && y >= 0 && y < H) {
            const size_t a = (size_t)y * (size_t)W + (size_t)x;
            c = cross_cell((double)MA[3 * a + 0], (double)MA[3 * a + 1], (double)MA[3 * a + 2], (double)MB[3 * a + 0],
                           (double)MB[3 * a + 1], (double)MB[3 * a + 2], se[a], scale);
        }
        sYa[i] = c.ya;
        sYb[i] = c.yb;
        sV[i] = c.v;
    }
    __syncthreads();

    const int px = tx0 + lx, py = ty0 + ly;
    const bool inside = px < W && py < H;
    // F_A's sums (weights of half B) and F_B's (weights of half A)
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, da = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, db = 0.0;
    int it = 0;
    for (int dy = -r; dy <= r; ++dy) {
        const int qy = py + dy;
        const int cnt_y = denoise_axis_count(py, dy, F, H);
        for (int dx = -r; dx <= r; ++dx, ++it) {
            double* const pa = planes + (it & 1) * (2 * PW * PS);
            double* const pb = pa + PW * PS;
            const bool centre = dx == 0 && dy == 0;
            if (!centre) {
                for (int i = tid; i < PW * PW; i += kThreads) {
                    const int cy = i / PW, cx = i - cy * PW;
                    const int ia = (cy + r) * SW + cx + r, ib = ia + dy * SW + dx;
                    const double va = sV[ia], vb = sV[ib];
                    double d_a = 0.0, d_b = 0.0;
                    if (!(va < 0.0) && !(vb < 0.0)) {
                        d_a = denoise_delta(sYa[ia], va, sYa[ib], vb, k2);
                        d_b = denoise_delta(sYb[ia], va, sYb[ib], vb, k2);
                    }
                    pa[cy * PS + cx] = d_a;
                    pb[cy * PS + cx] = d_b;
                }
            }
            __syncthreads();
            const int qx = px + dx;
            if (!inside || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            double wa = 1.0, wb = 1.0;
            if (!centre) {
                double s_a = 0.0, s_b = 0.0;
#pragma unroll
                for (int sy = 0; sy <= 2 * F; ++sy) {
#pragma unroll
                    for (int sx = 0; sx <= 2 * F; ++sx) {
                        s_a = s_a + pa[(ly + sy) * PS + lx + sx];
                        s_b = s_b + pb[(ly + sy) * PS + lx + sx];
                    }
                }
                const double cnt = (double)(denoise_axis_count(px, dx, F, W) * cnt_y);
                const double Da = s_a / cnt, Db = s_b / cnt;
                if constexpr (G) {
                    const double phi = denoise_phi(guides, (size_t)py * (size_t)W + (size_t)px,
                                                   (size_t)qy * (size_t)W + (size_t)qx);
                    wa = denoise_weight_guided(Da, phi);
                    wb = denoise_weight_guided(Db, phi);
                } else {
                    wa = denoise_weight(Da);
                    wb = denoise_weight(Db);
                }
            }
            const size_t b = (size_t)qy * (size_t)W + (size_t)qx;
            if (wb != 0.0) {
                a0 = a0 + wb * (double)MA[3 * b + 0];
                a1 = a1 + wb * (double)MA[3 * b + 1];
                a2 = a2 + wb * (double)MA[3 * b + 2];
                da = da + wb;
            }
            if (wa != 0.0) {
                b0 = b0 + wa * (double)MB[3 * b + 0];
                b1 = b1 + wa * (double)MB[3 * b + 1];
                b2 = b2 + wa * (double)MB[3 * b + 2];
                db = db + wa;
            }
        }
    }
    if (!inside) return;
    const int ic = (ly + h) * SW + lx + h;
    const size_t a = (size_t)py * (size_t)W + (size_t)px;
    double fa[3], fb[3];
    if (cross_bad(sYa[ic])) {
        for (int c = 0; c < 3; ++c) {
            fa[c] = (double)MA[3 * a + c];
            fb[c] = (double)MB[3 * a + c];
        }
    } else {
        fa[0] = a0 / da;
        fa[1] = a1 / da;
        fa[2] = a2 / da;
        fb[0] = b0 / db;
        fb[1] = b1 / db;
        fb[2] = b2 / db;
    }
    out[3 * a + 0] = (T)(0.5 * (fa[0] + fb[0]));
    out[3 * a + 1] = (T)(0.5 * (fa[1] + fb[1]));
    out[3 * a + 2] = (T)(0.5 * (fa[2] + fb[2]));
    if (e_out) e_out[a] = cross_half_diff(fa, fb);
}

// stderr_out from e: one thread per pixel
__global__ void __launch_bounds__(256) cross_stderr_map(const double* __restrict__ e, double* __restrict__ se_out, int W,
                                                         int H)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)W * (size_t)H) return;
    const int y = (int)(i / (size_t)W), x = (int)(i - (size_t)y * (size_t)W);
    se_out[i] = cross_stderr(e, x, y, W, H);
}

int cross_lds_bytes(int radius, int patch)
{
    const int sw = kCrossTile + 2 * (radius + patch), pw = kCrossTile + 2 * patch;
    return (3 * sw * sw + 4 * pw * cross_plane_stride(patch)) * (int)sizeof(double);
}

namespace {

struct CrossArgs {
    const void *mean_a, *mean_b;
    const double* se;
    void* out;
    double* e;
    int width, height, radius;
    double k, scale;
};

template <typename T, int F, bool G>
hipError_t launch_one(const CrossArgs& c, const DenoiseGuides& guides, hipStream_t stream)
{
    const int tiles_x = (c.width + kCrossTile - 1) / kCrossTile, tiles_y = (c.height + kCrossTile - 1) / kCrossTile;
    const long long tiles = (long long)tiles_x * tiles_y;
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((cross_nlm<T, F, G>), dim3((unsigned)tiles), dim3(kCrossTile * kCrossTile),
                       (size_t)cross_lds_bytes(c.radius, F), stream, (const T*)c.mean_a, (const T*)c.mean_b, c.se,
                       (T*)c.out, c.e, c.width, c.height, tiles_x, c.radius, c.k * c.k, c.scale, guides);
    return hipGetLastError();
}

template <typename T, bool G>
hipError_t launch_patch(const CrossArgs& c, int patch, const DenoiseGuides& guides, hipStream_t stream)
{
    switch (patch) {
    case 0: return launch_one<T, 0, G>(c, guides, stream);
    case 1: return launch_one<T, 1, G>(c, guides, stream);
    case 2: return launch_one<T, 2, G>(c, guides, stream);
    case 3: return launch_one<T, 3, G>(c, guides, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_cross(const void* mean_a, const void* mean_b, const double* se, void* out, double* se_out, double* e,
                        bool f64, int width, int height, int radius, int patch, double k, double scale,
                        const DenoiseGuides& guides, hipStream_t stream)
{
    if (width < 1 || height < 1 || radius < 1 || radius > kDenoiseMaxRadius || patch < 0 || patch > kDenoiseMaxPatch ||
        (se_out && !e))
        return hipErrorInvalidValue;
    const CrossArgs c{mean_a, mean_b, se, out, se_out ? e : nullptr, width, height, radius, k, scale};
    hipError_t rc;
    if (guides.any()) rc = f64 ? launch_patch<double, true>(c, patch, guides, stream) : launch_patch<float, true>(c, patch, guides, stream);
    else rc = f64 ? launch_patch<double, false>(c, patch, guides, stream) : launch_patch<float, false>(c, patch, guides, stream);
    if (rc != hipSuccess || !se_out) return rc;
    const size_t hw = (size_t)width * (size_t)height;
    hipLaunchKernelGGL(cross_stderr_map, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, stream, (const double*)e,
                       se_out, width, height);
    return hipGetLastError();
}

}  // namespace rtk
