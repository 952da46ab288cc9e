// adaptive_state_kernel.hpp — between the trace launches of an adaptive frame (rt_render_adaptive,
// rt_adaptive_state, rt_abi.h; adaptive_state_kernel.hip): the regroup kernel that chooses what a
// launch traces, and the mask of a caller's-map round. The rule is adaptive_schedule.hpp's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtk {

// What a regroup writes (u32 each), read back by the driver once per group
struct RegroupRecord {
    uint32_t n_group;    // tiles of the group (0: no tile is active)
    uint32_t n_star;     // their count (0 with an empty group)
    uint32_t n_active;   // active tiles, the group's included
    uint32_t n_min;      // the lowest and the highest count of any tile
    uint32_t n_max;
};

// order_out = [every other tile | the group], both parts in ascending raster index; the group =
// the active tiles of the lowest active count. Active: tile_spp < cap and (mask null: tile_spp == 0
// or not (threshold > 0 and tile_error <= threshold); mask: mask[t] != 0). With a mask the group's
// entries of it are cleared: a selected tile is stepped once. One workgroup; n_tiles >= 1.
hipError_t launch_adaptive_regroup(const uint32_t* tile_spp, const double* tile_error, uint32_t* mask,
                                   uint32_t* order_out, int n_tiles, double threshold, uint32_t cap,
                                   RegroupRecord* record, hipStream_t stream);

// mask[t] = tile_spp[t] < cap and not (threshold > 0 and error_in[t] <= threshold): the selected
// set of a caller's-map round
hipError_t launch_adaptive_select_mask(const uint32_t* tile_spp, const double* error_in, uint32_t* mask, int n_tiles,
                                       double threshold, uint32_t cap, hipStream_t stream);

}  // namespace rtk
