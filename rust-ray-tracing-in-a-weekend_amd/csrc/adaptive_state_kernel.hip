// adaptive_state_kernel.hip — what an adaptive frame's driver (adaptive_frame.cpp: rt_render_adaptive,
// rt_adaptive_state; rt_abi.h) launches between trace launches: the regroup step that chooses the
// tiles of the next launch, and the mask of a caller's-map round. The moments and the resolve are
// adaptive_kernel.hip's. The rule is stated on the host in adaptive_schedule.cpp.
#include "adaptive_state_kernel.hpp"

namespace rtk {

// One workgroup chooses the next group and writes the state's tile order as [every other tile |
// the group], each part in ascending raster index, in three sweeps over the tiles:
//   1. activity per tile; the lowest active count n*, the active tiles and the lowest and highest
//      count of all tiles: min / max by shuffles within a wave, counts by ballots, then across the
//      workgroup's waves through LDS (every thread reads the 16 wave values: a broadcast);
//   2. the size of the group (active and at n*), which fixes where the group starts;
//   3. the stable partition: ranks from ballots and popcounts within a wave and a prefix over the
//      waves' counts in LDS against a running base.
// No atomics: the order and the record are a function of tile_spp, the errors (or the mask), the
// threshold and the cap alone. With a mask, a tile placed in the group has its entry cleared (by
// the thread that read it), so a caller's-map round steps every selected tile once.
constexpr int kRegroupThreads = 1024;

__device__ __forceinline__ bool regroup_active(uint32_t n, double e, uint32_t m, bool by_mask, double threshold,
                                               uint32_t cap)
{
    return n < cap && (by_mask ? m != 0u : (n == 0u || !(threshold > 0.0 && e <= threshold)));
}

__global__ void __launch_bounds__(kRegroupThreads) adaptive_regroup(const uint32_t* __restrict__ tile_spp,
                                                                    const double* __restrict__ tile_error,
                                                                    uint32_t* __restrict__ mask,
                                                                    uint32_t* __restrict__ order_out, int n_tiles,
                                                                    double threshold, uint32_t cap,
                                                                    RegroupRecord* __restrict__ record)
{
    constexpr int kWaves = kRegroupThreads / 64;
    __shared__ unsigned w_a[kWaves], w_b[kWaves], w_c[kWaves], w_d[kWaves];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long below = lane ? ~0ULL >> (64 - lane) : 0ULL;   // the lanes before this one
    const bool by_mask = mask != nullptr;

    // sweep 1: n*, the active tiles, the range of the counts
    unsigned lo_active = ~0u, lo = ~0u, hi = 0u, n_active = 0u;
    for (int t0 = 0; t0 < n_tiles; t0 += kRegroupThreads) {
        const int t = t0 + tid;
        const bool valid = t < n_tiles;
        const uint32_t n = valid ? tile_spp[t] : 0u;
        const bool act = valid && regroup_active(n, by_mask ? 0.0 : tile_error[t], by_mask ? mask[t] : 0u, by_mask,
                                                 threshold, cap);
        n_active += (unsigned)__popcll(__ballot(act));   // (the wave's: the same in every lane)
        if (act) lo_active = min(lo_active, n);
        if (valid) {
            lo = min(lo, n);
            hi = max(hi, n);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo_active = min(lo_active, (unsigned)__shfl_xor((int)lo_active, d, 64));
        lo = min(lo, (unsigned)__shfl_xor((int)lo, d, 64));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, d, 64));
    }
    if (lane == 0) {
        w_a[w] = lo_active;
        w_b[w] = lo;
        w_c[w] = hi;
        w_d[w] = n_active;
    }
    __syncthreads();
    unsigned n_star = ~0u, n_min = ~0u, n_max = 0u, total_active = 0u;
    for (int i = 0; i < kWaves; ++i) {
        n_star = min(n_star, w_a[i]);
        n_min = min(n_min, w_b[i]);
        n_max = max(n_max, w_c[i]);
        total_active += w_d[i];
    }

    // sweep 2: the group's size
    unsigned mine = 0u;
    for (int t0 = 0; t0 < n_tiles; t0 += kRegroupThreads) {
        const int t = t0 + tid;
        const bool valid = t < n_tiles;
        const uint32_t n = valid ? tile_spp[t] : 0u;
        const bool in = valid && n == n_star &&
                        regroup_active(n, by_mask ? 0.0 : tile_error[t], by_mask ? mask[t] : 0u, by_mask, threshold, cap);
        mine += (unsigned)__popcll(__ballot(in));
    }
    __syncthreads();   // sweep 1's wave values are read
    if (lane == 0) w_a[w] = mine;
    __syncthreads();
    unsigned n_group = 0u;
    for (int i = 0; i < kWaves; ++i) n_group += w_a[i];

    // sweep 3: the partition
    unsigned base_rest = 0u, base_group = (unsigned)n_tiles - n_group;
    for (int t0 = 0; t0 < n_tiles; t0 += kRegroupThreads) {
        const int t = t0 + tid;
        const bool valid = t < n_tiles;
        const uint32_t n = valid ? tile_spp[t] : 0u;
        const bool in = valid && n == n_star &&
                        regroup_active(n, by_mask ? 0.0 : tile_error[t], by_mask ? mask[t] : 0u, by_mask, threshold, cap);
        const unsigned long long bg = __ballot(in), br = __ballot(valid && !in);
        __syncthreads();   // the previous round's (and sweep 2's) counts are read
        if (lane == 0) {
            w_a[w] = (unsigned)__popcll(bg);
            w_b[w] = (unsigned)__popcll(br);
        }
        __syncthreads();
        unsigned before_group = 0u, before_rest = 0u, round_group = 0u, round_rest = 0u;
        for (int i = 0; i < kWaves; ++i) {
            if (i < w) {
                before_group += w_a[i];
                before_rest += w_b[i];
            }
            round_group += w_a[i];
            round_rest += w_b[i];
        }
        if (in) {
            order_out[base_group + before_group + (unsigned)__popcll(bg & below)] = (uint32_t)t;
            if (by_mask) mask[t] = 0u;
        } else if (valid) {
            order_out[base_rest + before_rest + (unsigned)__popcll(br & below)] = (uint32_t)t;
        }
        base_group += round_group;
        base_rest += round_rest;
    }
    if (tid == 0) {
        record->n_group = n_group;
        record->n_star = n_group ? n_star : 0u;
        record->n_active = total_active;
        record->n_min = n_min;
        record->n_max = n_max;
    }
}

// One thread per tile.
__global__ void __launch_bounds__(256) adaptive_select_mask(const uint32_t* __restrict__ tile_spp,
                                                            const double* __restrict__ error_in,
                                                            uint32_t* __restrict__ mask, int n_tiles, double threshold,
                                                            uint32_t cap)
{
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n_tiles) return;
    mask[t] = (tile_spp[t] < cap && !(threshold > 0.0 && error_in[t] <= threshold)) ? 1u : 0u;
}

hipError_t launch_adaptive_regroup(const uint32_t* tile_spp, const double* tile_error, uint32_t* mask,
                                   uint32_t* order_out, int n_tiles, double threshold, uint32_t cap,
                                   RegroupRecord* record, hipStream_t stream)
{
    if (n_tiles <= 0 || !tile_spp || !order_out || !record || (!tile_error && !mask)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adaptive_regroup, dim3(1), dim3(kRegroupThreads), 0, stream, tile_spp, tile_error, mask,
                       order_out, n_tiles, threshold, cap, record);
    return hipGetLastError();
}

hipError_t launch_adaptive_select_mask(const uint32_t* tile_spp, const double* error_in, uint32_t* mask, int n_tiles,
                                       double threshold, uint32_t cap, hipStream_t stream)
{
    if (n_tiles <= 0 || !tile_spp || !error_in || !mask) return hipErrorInvalidValue;
    hipLaunchKernelGGL(adaptive_select_mask, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, stream, tile_spp,
                       error_in, mask, n_tiles, threshold, cap);
    return hipGetLastError();
}

}  // namespace rtk
