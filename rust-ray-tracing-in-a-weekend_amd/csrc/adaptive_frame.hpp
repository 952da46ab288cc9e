// adaptive_frame.hpp — the device side of an adaptive frame, owned, and its one driver: what
// rt_render_adaptive(_halves) keeps for a call (abi_passes.cpp) and rt_adaptive_state between calls
// (abi_adaptive_state.cpp). The block's layout is stated here and nowhere else; what a launch
// traces is chosen on the device (adaptive_state_kernel.hip) by the rule of adaptive_schedule.hpp.
// Private to the library, as render_internal.hpp is.
#pragma once

#include "adaptive_schedule.hpp"
#include "adaptive_state_kernel.hpp"
#include "ctx_internal.hpp"
#include "trace_kernel.hpp"

#pragma GCC visibility push(hidden)

// One allocation, zeroed at init: [sum | sum_open | q | q_open | tile_error | a caller's map |
// halves: sum_a | sum_a_open | sum_b | sum_b_open] f64, then [tile_spp | order | mask | the regroup
// record] u32. Offsets in elements of their part.
struct AdaptiveLayout {
    size_t hw, nt;   // pixels, tiles
    size_t sum, sum_open, q, q_open, tile_error, error_in, sum_a, sum_a_open, sum_b, sum_b_open, n_f64;
    size_t tile_spp, order, mask, record, n_u32;

    AdaptiveLayout(int width, int height, bool with_halves)
    {
        hw = (size_t)width * (size_t)height;
        nt = (size_t)((width + 7) / 8) * (size_t)((height + 7) / 8);
        size_t at = 0;
        auto take = [&at](size_t n) { const size_t o = at; at += n; return o; };
        sum = take(3 * hw), sum_open = take(3 * hw), q = take(hw), q_open = take(hw);
        tile_error = take(nt), error_in = take(nt);
        const size_t half = with_halves ? 3 * hw : 0;
        sum_a = take(half), sum_a_open = take(half), sum_b = take(half), sum_b_open = take(half);
        n_f64 = at;
        at = 0;
        tile_spp = take(nt), order = take(nt), mask = take(nt);
        record = take(sizeof(rtk::RegroupRecord) / sizeof(uint32_t));
        n_u32 = at;
    }
    size_t bytes() const { return n_f64 * sizeof(double) + n_u32 * sizeof(uint32_t); }
};

// What one advance did: what rt_adaptive_stats, rt_adaptive_state_stats and rt_last_stats need of it
struct AdaptiveAdvance {
    int launches = 0, batches = 0, max_launch_batches = 0;   // trace launches: of the call, the most of one launch
    uint64_t samples = 0;
    double trace_ms = 0.0, moments_ms = 0.0, classify_ms = 0.0;   // classify: the regroups with their readbacks
    int32_t active_left = 0;
};

struct AdaptiveBlock {
    int width = 0, height = 0, n_tiles = 0;
    bool with_halves = false;
    DevBuf blk;
    rtk::AdaptiveFrame F{};
    rtk::AdaptiveHalves Hf{};
    uint32_t* order = nullptr;       // [every other tile | the group]
    uint32_t* mask = nullptr;        // a caller's-map round: the tiles still to step
    double* error_in = nullptr;      //   its map, when the caller's is on the host
    rtk::RegroupRecord* record = nullptr;
    EventSpan<2> ev;                 // around a regroup and its readback
    // the host side
    bool order_is_raster = true;     // no regroup has run: the order is the one init wrote
    int ragged_cap = 0;              // 0, or the cap at which a launch closed a partial chunk
    uint32_t min_count = 0, max_count = 0;

    // Allocates and zeroes the block and writes the raster order. on_stream given: with the async
    // calls on it and one synchronization (a call that keeps all its work on its stream); null:
    // with the blocking calls of the null stream.
    hipError_t init(int width, int height, bool with_halves, const hipStream_t* on_stream);

    // Launches groups until no tile is active under (threshold, cap) or max_launches (0: no limit)
    // are done; map (null: the frame's own tile errors) selects the tiles of a caller's-map round.
    // rp: a launch's params but for its tile range and sample count. `a` is filled on every way out.
    int advance(rt_ctx* c, const rt_camera* cam, const rt_render_params& rp, const rtas::Schedule& s, double threshold,
                int cap, int max_launches, const double* map, bool map_on_device, hipStream_t stream, AdaptiveAdvance& a);

    // Enqueues the resolve into the caller's outputs (hv null: no half means); host-bound ones are
    // staged in `stage`, grown as needed. The caller synchronizes.
    int resolve(int out_format, bool on_device, const rt_adaptive_out* out, const rt_adaptive_halves* hv, DevBuf& stage,
                hipStream_t stream);
};

// rt_last_stats after an advance: the call as a whole (the variant fields are the last launch's)
void adaptive_last_stats(rt_ctx* c, const AdaptiveAdvance& a, int cap, int chunk, int n_tiles);

#pragma GCC visibility pop
