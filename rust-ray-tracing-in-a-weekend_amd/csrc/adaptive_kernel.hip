// adaptive_kernel.hip — the kernels of tile-adaptive sampling (rt_render_adaptive): the moments
// reduction over a pass's per-sample records and the resolve. The criterion itself is
// adaptive_criterion.hpp; the regroup step that re-deals the tiles between passes is
// adaptive_state_kernel.hip's.
#include "adaptive_criterion.hpp"
#include "trace_kernel.hpp"

namespace rtk {

// reduce_samples_carry's contract with a second moment, organised as reduce_samples_tiled: one
// workgroup per tile of the shard, wave w of kMomentWaves sums chunk segments w, w + W, ... of
// the tile's 64 pixels (four samples' loads in flight, each wave reading the tile's 64
// consecutive records of a sample), parks the segment sums in LDS, and wave 0 adds a round's
// segments in order to the running totals: rt_render's additions in rt_render's order.
//
// A batch holds samples [0, n_samples) of which the first continues a chunk `pos` samples in
// (its sum so far in *_open); segment k covers the batch's samples of chunk k counted from that
// chunk's start. A segment that reaches its chunk's end (or the pass's end, `close`) is added to
// the closed totals; the last one otherwise goes back to *_open. Shard tile m is the raster tile
// order[pos_begin + m], and the totals are in frame layout (row 0 = bottom, as rt_render's out).
// On `close` wave 0 also evaluates the criterion with n_done samples per pixel, sums e_px over the
// tile's in-image pixels across its 64 lanes and writes tile_error / tile_spp of the raster tile.
//
// HV (rt_render_adaptive_halves): the same launch also sums the RGB of the samples with an even
// global index (first + j: half a) and of those with an odd one (half b), exactly as it sums all of
// them: per segment from 0.0 (or the half's open chunk) in sample order, the segments in order onto
// Hf's totals. Six more accumulators per lane and per LDS segment slot (part[8][10][64], 40 KB).
// Without HV nothing of it is compiled: rt_render_adaptive's instantiation.
constexpr int kMomentWaves = 8;
template <bool HV>
__global__ void __launch_bounds__(64 * kMomentWaves) adaptive_moments(const double* __restrict__ samples,
                                                                       AdaptiveFrame F, int n_samples, int chunk,
                                                                       int pos, int close, int n_done,
                                                                       AdaptiveHalves Hf, int first)
{
    __shared__ double part[kMomentWaves][HV ? 10 : 4][64];
    const unsigned m = blockIdx.x;
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const unsigned t = F.order[(size_t)F.pos_begin + m];
    const int tx = (int)(t % (unsigned)F.tiles_x), ty = (int)(t / (unsigned)F.tiles_x);
    const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
    const bool inside = x < F.width && y < F.height;
    const size_t px = inside ? (size_t)y * (size_t)F.width + (size_t)x : 0;
    const double* base = samples + ((size_t)m * (size_t)n_samples * 64 + (size_t)lane) * 3;
    const int n_seg = (n_samples + pos + chunk - 1) / chunk;
    double r = 0.0, g = 0.0, b = 0.0, q = 0.0;          // wave 0: the closed chunks' totals
    double o_r = 0.0, o_g = 0.0, o_b = 0.0, o_q = 0.0;  // wave 0: the chunk left open
    double ha[3] = {0.0, 0.0, 0.0}, hb[3] = {0.0, 0.0, 0.0};       // HV, wave 0: the halves' closed totals
    double oa[3] = {0.0, 0.0, 0.0}, ob[3] = {0.0, 0.0, 0.0};       // HV, wave 0: their open chunk
    if (w == 0 && inside) {
        r = F.sum[3 * px + 0];
        g = F.sum[3 * px + 1];
        b = F.sum[3 * px + 2];
        q = F.q[px];
        if constexpr (HV) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ha[c] = Hf.sum_a[3 * px + c];
                hb[c] = Hf.sum_b[3 * px + c];
            }
        }
    }
    for (int k0 = 0; k0 < n_seg; k0 += kMomentWaves) {
        const int k = k0 + w;
        if (k < n_seg) {
            const int j0 = max(0, k * chunk - pos), j1 = min(n_samples, (k + 1) * chunk - pos);
            double cr = 0.0, cg = 0.0, cb = 0.0, cq = 0.0;
            double ca[3] = {0.0, 0.0, 0.0}, cb2[3] = {0.0, 0.0, 0.0};   // HV: the segment's half sums
            if (k == 0 && pos > 0 && inside) {
                cr = F.sum_open[3 * px + 0];
                cg = F.sum_open[3 * px + 1];
                cb = F.sum_open[3 * px + 2];
                cq = F.q_open[px];
                if constexpr (HV) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        ca[c] = Hf.sum_a_open[3 * px + c];
                        cb2[c] = Hf.sum_b_open[3 * px + c];
                    }
                }
            }
            int j = j0;
            for (; j + 4 <= j1; j += 4) {
                double v[4][3];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double* p = base + (size_t)(j + i) * 192;
                    v[i][0] = p[0];
                    v[i][1] = p[1];
                    v[i][2] = p[2];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double yl = adaptive_luma(v[i][0], v[i][1], v[i][2]);
                    cr = cr + v[i][0];
                    cg = cg + v[i][1];
                    cb = cb + v[i][2];
                    cq = cq + yl * yl;
                    if constexpr (HV) {   // (the parity is the wave's: no lane diverges)
                        if (((first + j + i) & 1) == 0) {
                            ca[0] = ca[0] + v[i][0];
                            ca[1] = ca[1] + v[i][1];
                            ca[2] = ca[2] + v[i][2];
                        } else {
                            cb2[0] = cb2[0] + v[i][0];
                            cb2[1] = cb2[1] + v[i][1];
                            cb2[2] = cb2[2] + v[i][2];
                        }
                    }
                }
            }
            for (; j < j1; ++j) {
                const double* p = base + (size_t)j * 192;
                const double v0 = p[0], v1 = p[1], v2 = p[2];
                const double yl = adaptive_luma(v0, v1, v2);
                cr = cr + v0;
                cg = cg + v1;
                cb = cb + v2;
                cq = cq + yl * yl;
                if constexpr (HV) {
                    if (((first + j) & 1) == 0) {
                        ca[0] = ca[0] + v0;
                        ca[1] = ca[1] + v1;
                        ca[2] = ca[2] + v2;
                    } else {
                        cb2[0] = cb2[0] + v0;
                        cb2[1] = cb2[1] + v1;
                        cb2[2] = cb2[2] + v2;
                    }
                }
            }
            part[w][0][lane] = cr;
            part[w][1][lane] = cg;
            part[w][2][lane] = cb;
            part[w][3][lane] = cq;
            if constexpr (HV) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    part[w][4 + c][lane] = ca[c];
                    part[w][7 + c][lane] = cb2[c];
                }
            }
        }
        __syncthreads();
        if (w == 0) {
            const int nk = min(kMomentWaves, n_seg - k0);
            for (int i = 0; i < nk; ++i) {
                const bool closed = (k0 + i + 1) * chunk - pos <= n_samples || close;
                if (closed) {
                    r = r + part[i][0][lane];
                    g = g + part[i][1][lane];
                    b = b + part[i][2][lane];
                    q = q + part[i][3][lane];
                    if constexpr (HV) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            ha[c] = ha[c] + part[i][4 + c][lane];
                            hb[c] = hb[c] + part[i][7 + c][lane];
                        }
                    }
                } else {   // the batch's last segment, its chunk continued by the next batch
                    o_r = part[i][0][lane];
                    o_g = part[i][1][lane];
                    o_b = part[i][2][lane];
                    o_q = part[i][3][lane];
                    if constexpr (HV) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            oa[c] = part[i][4 + c][lane];
                            ob[c] = part[i][7 + c][lane];
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (w != 0) return;
    if (inside) {
        F.sum[3 * px + 0] = r;
        F.sum[3 * px + 1] = g;
        F.sum[3 * px + 2] = b;
        F.q[px] = q;
        if (!close) {
            F.sum_open[3 * px + 0] = o_r;
            F.sum_open[3 * px + 1] = o_g;
            F.sum_open[3 * px + 2] = o_b;
            F.q_open[px] = o_q;
        }
        if constexpr (HV) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Hf.sum_a[3 * px + c] = ha[c];
                Hf.sum_b[3 * px + c] = hb[c];
                if (!close) {
                    Hf.sum_a_open[3 * px + c] = oa[c];
                    Hf.sum_b_open[3 * px + c] = ob[c];
                }
            }
        }
    }
    if (!close) return;
    double e = inside ? adaptive_pixel_noise(r, g, b, q, (double)n_done).e : 0.0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) e = e + __shfl_xor(e, d, 64);   // every lane: the same sum
    if (lane == 0) {
        const int cw = min(8, F.width - tx * 8), ch = min(8, F.height - ty * 8);
        F.tile_error[t] = e / (double)(cw * ch);
        F.tile_spp[t] = (uint32_t)n_done;
    }
}

// mean = sum * (1 / the tile's sample count), as rt_render writes it, and (se_map not null) the
// standard error of each pixel's luminance mean. One thread per pixel of the frame.
template <typename T>
__global__ void __launch_bounds__(256) adaptive_resolve(const double* __restrict__ sum, const double* __restrict__ q,
                                                        const uint32_t* __restrict__ tile_spp, T* __restrict__ mean,
                                                        double* __restrict__ se_map, int width, int height,
                                                        int tiles_x)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)width * height) return;
    const int y = (int)(i / width), x = (int)(i - (long long)y * width);
    const double n = (double)tile_spp[(size_t)(y >> 3) * (size_t)tiles_x + (size_t)(x >> 3)];
    const double scale = 1.0 / n;
    const double r = sum[3 * i + 0], g = sum[3 * i + 1], b = sum[3 * i + 2];
    mean[3 * i + 0] = (T)(r * scale);
    mean[3 * i + 1] = (T)(g * scale);
    mean[3 * i + 2] = (T)(b * scale);
    if (se_map) se_map[i] = adaptive_pixel_noise(r, g, b, q[i], n).se;
}

hipError_t launch_adaptive_moments(const double* samples, const AdaptiveFrame& F, int n_tiles, int n_samples,
                                   int chunk, int pos, bool close, int n_done, hipStream_t stream,
                                   const AdaptiveHalves* halves, int first)
{
    if (n_tiles <= 0 || n_samples <= 0) return hipSuccess;
    if (chunk < 1 || pos < 0 || pos >= chunk || n_done < 2 || first < 0) return hipErrorInvalidValue;
    if (halves)
        hipLaunchKernelGGL(adaptive_moments<true>, dim3((unsigned)n_tiles), dim3(64 * kMomentWaves), 0, stream, samples,
                           F, n_samples, chunk, pos, (int)close, n_done, *halves, first);
    else
        hipLaunchKernelGGL(adaptive_moments<false>, dim3((unsigned)n_tiles), dim3(64 * kMomentWaves), 0, stream, samples,
                           F, n_samples, chunk, pos, (int)close, n_done, AdaptiveHalves{}, 0);
    return hipGetLastError();
}

// the two half means of rt_render_adaptive_halves. One thread per pixel of the frame.
template <typename T>
__global__ void __launch_bounds__(256) adaptive_resolve_halves(const double* __restrict__ sum_a,
                                                               const double* __restrict__ sum_b,
                                                               const uint32_t* __restrict__ tile_spp,
                                                               T* __restrict__ mean_a, T* __restrict__ mean_b, int width,
                                                               int height, int tiles_x)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)width * height) return;
    const int y = (int)(i / width), x = (int)(i - (long long)y * width);
    const uint32_t n = tile_spp[(size_t)(y >> 3) * (size_t)tiles_x + (size_t)(x >> 3)];
    const double sa = 1.0 / (double)((n + 1u) / 2u), sb = 1.0 / (double)(n / 2u);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        mean_a[3 * i + c] = (T)(sum_a[3 * i + c] * sa);
        mean_b[3 * i + c] = (T)(sum_b[3 * i + c] * sb);
    }
}

hipError_t launch_adaptive_resolve(const double* sum, const double* q, const uint32_t* tile_spp, void* mean, bool f64,
                                   double* se_map, int width, int height, hipStream_t stream)
{
    const long long blocks = ((long long)width * height + 255) / 256;
    if (blocks <= 0) return hipSuccess;
    const int tiles_x = (width + 7) / 8;
    if (f64)
        hipLaunchKernelGGL(adaptive_resolve<double>, dim3((unsigned)blocks), dim3(256), 0, stream, sum, q, tile_spp,
                           (double*)mean, se_map, width, height, tiles_x);
    else
        hipLaunchKernelGGL(adaptive_resolve<float>, dim3((unsigned)blocks), dim3(256), 0, stream, sum, q, tile_spp,
                           (float*)mean, se_map, width, height, tiles_x);
    return hipGetLastError();
}

hipError_t launch_adaptive_resolve_halves(const double* sum_a, const double* sum_b, const uint32_t* tile_spp,
                                          void* mean_a, void* mean_b, bool f64, int width, int height,
                                          hipStream_t stream)
{
    const long long blocks = ((long long)width * height + 255) / 256;
    if (blocks <= 0) return hipSuccess;
    const int tiles_x = (width + 7) / 8;
    if (f64)
        hipLaunchKernelGGL(adaptive_resolve_halves<double>, dim3((unsigned)blocks), dim3(256), 0, stream, sum_a, sum_b,
                           tile_spp, (double*)mean_a, (double*)mean_b, width, height, tiles_x);
    else
        hipLaunchKernelGGL(adaptive_resolve_halves<float>, dim3((unsigned)blocks), dim3(256), 0, stream, sum_a, sum_b,
                           tile_spp, (float*)mean_a, (float*)mean_b, width, height, tiles_x);
    return hipGetLastError();
}

}  // namespace rtk
