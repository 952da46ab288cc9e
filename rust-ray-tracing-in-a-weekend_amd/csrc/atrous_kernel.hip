// atrous_kernel.hip — the device half of rt_denoise_atrous (include/rt/rt_abi.h): the
// variance-guided a-trous wavelet filter over a mean frame, its standard-error map and optional
// first-hit guides. The arithmetic is atrous_core.hpp's, shared with the host filter
// (atrous_host.cpp).
//
// One launch per level, each an instantiation over (first, last, guided, T):
//   first  reads M and se (and the albedo when demodulated) and forms state 0 in the load:
//          widening and demodulation cost no pass of their own
//   last   writes out and stderr_out: re-modulation and the rounding to T are in the store
//   else   reads and writes frames of 32-byte state records (c0, c1, c2, V): a tap is two 16-byte
//          loads, Y is recomputed from the record
// so L = 1 needs no state buffer, L = 2 one, and L >= 3 two that alternate.
//
// Steps 4 and up: one pixel per thread, direct gather, no LDS (atrous_level_kernel). A 256-thread
// workgroup is a 64 x 4 tile, a wave one row of 64 consecutive x. For a fixed tap the offset
// s (dx, dy) is the same in every lane, so the lanes read 64 consecutive records (2 KB) whatever
// the step: the gather is coalesced at every level, and what a larger step costs is reuse between
// neighbouring workgroups in L2, not transactions. Vbar's nine V values are read the same way at
// distance 1. Steps 1 and 2: the state of a 32 x 8 tile and its halo staged once in LDS
// (atrous_level_tiled, below), which measured faster at both. Every access is
// behind its pixel's inside-the-image test (atrous_core.hpp). No atomics and no cross-workgroup
// state: a pixel's sums depend on state i alone, in raster tap order, whatever the tiling, so the
// result repeats bit for bit, and both kernels give the same bits.
#include "atrous.hpp"
#include "atrous_core.hpp"

namespace rtk {

constexpr int kAtrousTileW = 64, kAtrousTileH = 4;

// The steps (0: none; 1; 2: 1 and 2) whose levels take the LDS-staged kernel instead of the direct
// gather. 2 is the measured choice; the others are for A/B builds (scripts/atrous_ab.py).
#ifndef RT_ATROUS_LDS_STEPS
#define RT_ATROUS_LDS_STEPS 2
#endif

// state 0, formed from the inputs at every read
template <typename T>
struct AtrousFirstAccess {
    const T* M;
    const double* se;
    const double* albedo;   // null: not demodulated
    int W;
    __device__ AtrousRec load(int x, int y) const
    {
        const size_t i = (size_t)y * (size_t)W + (size_t)x;
        return atrous_initial((double)M[3 * i], (double)M[3 * i + 1], (double)M[3 * i + 2], se[i],
                              albedo ? albedo + 3 * i : nullptr);
    }
    __device__ double var(int x, int y) const
    {
        const size_t i = (size_t)y * (size_t)W + (size_t)x;
        return atrous_initial(0.0, 0.0, 0.0, se[i], albedo ? albedo + 3 * i : nullptr).v;
    }
};

struct AtrousStateAccess {
    const AtrousRec* s;
    int W;
    __device__ AtrousRec load(int x, int y) const { return s[(size_t)y * (size_t)W + (size_t)x]; }
    __device__ double var(int x, int y) const { return s[(size_t)y * (size_t)W + (size_t)x].v; }
};

// what a thread does with its pixel's new state: the next level's record, or the call's outputs
template <bool LAST, typename T>
__device__ inline void atrous_store(const AtrousRec& r, size_t p, const T* __restrict__ M, const double* __restrict__ se,
                                    const double* albedo, AtrousRec* __restrict__ state_out, T* __restrict__ out,
                                    double* __restrict__ se_out)
{
    if constexpr (!LAST) {
        state_out[p] = r;
    } else {
        double c[3], e;
        atrous_final(r, albedo ? albedo + 3 * p : nullptr, c, e);
        const T m0 = M[3 * p + 0], m1 = M[3 * p + 1], m2 = M[3 * p + 2];
        const bool keep = !denoise_finite(denoise_luma((double)m0, (double)m1, (double)m2)) || !denoise_finite(se[p]);
        out[3 * p + 0] = keep ? m0 : (T)c[0];
        out[3 * p + 1] = keep ? m1 : (T)c[1];
        out[3 * p + 2] = keep ? m2 : (T)c[2];
        if (se_out) se_out[p] = e;
    }
}

template <bool FIRST, bool LAST, bool G, typename T>
__global__ void __launch_bounds__(kAtrousTileW* kAtrousTileH)
    atrous_level_kernel(const T* __restrict__ M, const double* __restrict__ se, const double* albedo,
                        const AtrousRec* __restrict__ in, AtrousRec* __restrict__ state_out, T* __restrict__ out,
                        double* __restrict__ se_out, int W, int H, int tiles_x, int s, double sigma_l,
                        DenoiseGuides guides)
{
    const int tid = (int)threadIdx.x;
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * kAtrousTileW + (tid & (kAtrousTileW - 1));
    const int y = (int)(blockIdx.x / (unsigned)tiles_x) * kAtrousTileH + tid / kAtrousTileW;
    if (x >= W || y >= H) return;
    AtrousRec r;
    if constexpr (FIRST) r = atrous_level<G>(AtrousFirstAccess<T>{M, se, albedo, W}, guides, x, y, W, H, s, sigma_l);
    else r = atrous_level<G>(AtrousStateAccess{in, W}, guides, x, y, W, H, s, sigma_l);
    atrous_store<LAST, T>(r, (size_t)y * (size_t)W + (size_t)x, M, se, albedo, state_out, out, se_out);
}

// ---- the LDS-staged variant, steps 1 and 2 (RT_ATROUS_LDS_STEPS) ----------------------------------
// A 32 x 8 tile and its halo of 2 S pixels, (32 + 4 S) x (8 + 4 S) cells, staged once as four planes of
// doubles (c0, c1, c2, V: a wave row's 32 lanes read 32 consecutive doubles of a plane, all 64 banks
// once): 13.8 KB at S = 1, 20.5 KB at S = 2. State 0 is then formed once per cell, not once per
// tap. At step 4 the halo (16) would be larger than the tile. Cells outside the image are neither
// staged nor read: every read is behind atrous_core.hpp's inside test, and a tap or Vbar neighbour
// of a tile pixel lies within the halo. The values are the direct gather's, so are the bits.
constexpr int kAtrousLdsTileW = 32, kAtrousLdsTileH = 8;

template <int TW, int CELLS>
struct AtrousTileAccess {
    const double* t;   // 4 planes of CELLS doubles
    int x0, y0;        // the image position of cell (0, 0)
    __device__ AtrousRec load(int x, int y) const
    {
        const int i = (y - y0) * TW + (x - x0);
        AtrousRec r;
        r.c0 = t[i];
        r.c1 = t[CELLS + i];
        r.c2 = t[2 * CELLS + i];
        r.v = t[3 * CELLS + i];
        return r;
    }
    __device__ double var(int x, int y) const { return t[3 * CELLS + (y - y0) * TW + (x - x0)]; }
};

template <bool FIRST, bool LAST, bool G, typename T, int S>
__global__ void __launch_bounds__(kAtrousLdsTileW* kAtrousLdsTileH)
    atrous_level_tiled(const T* __restrict__ M, const double* __restrict__ se, const double* albedo,
                       const AtrousRec* __restrict__ in, AtrousRec* __restrict__ state_out, T* __restrict__ out,
                       double* __restrict__ se_out, int W, int H, int tiles_x, double sigma_l, DenoiseGuides guides)
{
    constexpr int kThreads = kAtrousLdsTileW * kAtrousLdsTileH, HALO = 2 * S;
    constexpr int TW = kAtrousLdsTileW + 2 * HALO, TH = kAtrousLdsTileH + 2 * HALO, CELLS = TW * TH;
    __shared__ double tile[4 * CELLS];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * kAtrousLdsTileW - HALO;
    const int y0 = (int)(blockIdx.x / (unsigned)tiles_x) * kAtrousLdsTileH - HALO;
    for (int i = tid; i < CELLS; i += kThreads) {
        const int cy = i / TW, cx = i - cy * TW;
        const int x = x0 + cx, y = y0 + cy;
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
        AtrousRec r;
        if constexpr (FIRST) r = AtrousFirstAccess<T>{M, se, albedo, W}.load(x, y);
        else r = in[(size_t)y * (size_t)W + (size_t)x];
        tile[i] = r.c0;
        tile[CELLS + i] = r.c1;
        tile[2 * CELLS + i] = r.c2;
        tile[3 * CELLS + i] = r.v;
    }
    __syncthreads();
    const int x = x0 + HALO + (tid & (kAtrousLdsTileW - 1)), y = y0 + HALO + tid / kAtrousLdsTileW;
    if (x >= W || y >= H) return;
    const AtrousRec r = atrous_level<G>(AtrousTileAccess<TW, CELLS>{tile, x0, y0}, guides, x, y, W, H, S, sigma_l);
    atrous_store<LAST, T>(r, (size_t)y * (size_t)W + (size_t)x, M, se, albedo, state_out, out, se_out);
}

namespace {

struct AtrousCall {
    const void* mean;
    const double* se;
    const double* albedo;
    void* out;
    double* se_out;
    int W, H;
    double sigma_l;
    DenoiseGuides guides;
    hipStream_t stream;
};

template <bool FIRST, bool LAST, bool G, typename T>
hipError_t launch_level(const AtrousCall& c, const AtrousRec* in, AtrousRec* state_out, int s)
{
    // step 1 is the first level's and step 2 the second's, so each pair (FIRST, step) has one tiled instantiation
    constexpr int S = FIRST ? 1 : 2;
    const bool tiled = s == S && s <= RT_ATROUS_LDS_STEPS;
    const int tw = tiled ? kAtrousLdsTileW : kAtrousTileW, th = tiled ? kAtrousLdsTileH : kAtrousTileH;
    const int tiles_x = (c.W + tw - 1) / tw, tiles_y = (c.H + th - 1) / th;
    const long long tiles = (long long)tiles_x * tiles_y;
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    if (tiled)
        hipLaunchKernelGGL((atrous_level_tiled<FIRST, LAST, G, T, S>), dim3((unsigned)tiles),
                           dim3(kAtrousLdsTileW * kAtrousLdsTileH), 0, c.stream, (const T*)c.mean, c.se, c.albedo, in,
                           state_out, (T*)c.out, c.se_out, c.W, c.H, tiles_x, c.sigma_l, c.guides);
    else
        hipLaunchKernelGGL((atrous_level_kernel<FIRST, LAST, G, T>), dim3((unsigned)tiles),
                           dim3(kAtrousTileW * kAtrousTileH), 0, c.stream, (const T*)c.mean, c.se, c.albedo, in, state_out,
                           (T*)c.out, c.se_out, c.W, c.H, tiles_x, s, c.sigma_l, c.guides);
    return hipGetLastError();
}

template <bool G, typename T>
hipError_t launch_levels(const AtrousCall& c, int levels, AtrousRec* scratch)
{
    const size_t hw = (size_t)c.W * (size_t)c.H;
    AtrousRec* const buf[2] = {scratch, scratch ? scratch + hw : nullptr};
    if (levels == 1) return launch_level<true, true, G, T>(c, nullptr, nullptr, 1);
    hipError_t e = launch_level<true, false, G, T>(c, nullptr, buf[0], 1);
    for (int i = 1; i < levels - 1 && e == hipSuccess; ++i)
        e = launch_level<false, false, G, T>(c, buf[(i - 1) & 1], buf[i & 1], 1 << i);
    if (e != hipSuccess) return e;
    return launch_level<false, true, G, T>(c, buf[(levels - 2) & 1], nullptr, 1 << (levels - 1));
}

}  // namespace

hipError_t launch_atrous(const void* mean, const double* se, void* out, double* stderr_out, bool f64, int width,
                         int height, int levels, double sigma_l, const double* albedo, const DenoiseGuides& guides,
                         AtrousRec* scratch, hipStream_t stream)
{
    if (width < 1 || height < 1 || levels < 1 || levels > kAtrousMaxLevels || (levels > 1 && !scratch))
        return hipErrorInvalidValue;
    const AtrousCall c{mean, se, albedo, out, stderr_out, width, height, sigma_l, guides, stream};
    if (guides.any()) return f64 ? launch_levels<true, double>(c, levels, scratch) : launch_levels<true, float>(c, levels, scratch);
    return f64 ? launch_levels<false, double>(c, levels, scratch) : launch_levels<false, float>(c, levels, scratch);
}

}  // namespace rtk
