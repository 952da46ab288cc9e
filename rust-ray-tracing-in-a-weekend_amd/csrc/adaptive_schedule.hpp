// adaptive_schedule.hpp — the host side of an adaptive frame (rt_render_adaptive, rt_adaptive_state;
// rt_abi.h): the schedule of counts, the rounding to the chunk, the ragged-cap rule, the checks of
// the one-shot call, create, advance and restore, and the selection rule of a group. Pure
// arithmetic, no HIP and no context, as launch_plan.hpp: adaptive_frame.cpp enqueues what it
// decides, tests/adaptive_schedule_main.cpp runs it on a CPU. The only statement of the selection
// rule outside adaptive_state_kernel.hip.
#pragma once

#include <cstdint>

#include "rt/rt_abi.h"

namespace rtas {

// v rounded up to a multiple of chunk (chunk >= 1), at most INT32_MAX rounded down to one
int round_up(int v, int chunk);

// next(n) = min(cap, n == 0 ? min_r : n + step_r)
int next_count(int64_t n, int cap, int min_r, int step_r);

// rt_render_adaptive's stop predicate: a threshold <= 0 stops no tile, nor does a NaN error
inline bool stops(double e, double threshold) { return threshold > 0.0 && e <= threshold; }

// tile with count n and error e under (threshold, cap)
inline bool active(uint32_t n, double e, double threshold, int cap)
{
    return n < (uint32_t)cap && (n == 0 || !stops(e, threshold));
}

// What an adaptive frame is driven with, as rounded
struct Schedule {
    int chunk = 1, min_r = 2, step_r = 1;
};

// Each check returns nullptr, or the text of the RT_ERR_INVALID it stands for.
// create and the one-shot call: p's geometry and shard fields, ap's min_spp / step_spp; fill s
// (auto_chunk: rt_render's automatic chunk for p->spp, taken when p->spp_chunk is 0). A state
// rounds min_spp and step_spp to the chunk it is given. The one-shot call also needs p->spp >= 2,
// an out_format and a threshold that is not NaN; its chunk is at most p->spp, as rt_render's, and
// its rounded min_spp and step_spp are capped at p->spp.
const char* check_create(const rt_render_params* p, const rt_adaptive_params* ap, int auto_chunk, Schedule& s);
const char* check_one_shot(const rt_render_params* p, const rt_adaptive_params* ap, int auto_chunk, Schedule& s);
// advance: a's fields against the state's host side: ragged_cap (0: none) and whether a tile is at count 0
const char* check_advance(const rt_adaptive_advance_params* a, int ragged_cap, bool any_zero);
// A launch to `end` samples under the chunk: the ragged cap after it (end itself when it closes a
// partial chunk, else what it was)
int ragged_after(int ragged_cap, int end, int chunk);
// restore: the header against the state's own, and every count against the chunk grid
const char* check_restore(const rt_adaptive_state_header* h, const uint32_t* tile_spp, int64_t n_tiles, int width,
                          int height, const Schedule& s, bool with_halves);

// The selection rule (rt_abi.h: rt_adaptive_next_group_host). tile_error or selected, not both.
rt_adaptive_group next_group(const uint32_t* tile_spp, const double* tile_error, const uint8_t* selected,
                             int64_t n_tiles, double threshold, int cap, int min_r, int step_r, uint32_t* group_out);

}  // namespace rtas
