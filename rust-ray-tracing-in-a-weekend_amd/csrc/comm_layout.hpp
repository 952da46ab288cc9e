// comm_layout.hpp — the one statement of what rt_render_gather moves between ranks (comm.cpp):
// a rank's tile slab with its status trailer, where rank r's slab and trailer lie in rank 0's
// gathered buffer, the element stride the reorder kernel (trace_kernel.hip, assemble_tiles)
// steps from rank to rank, and the reading of the gathered status words. Nothing from HIP:
// tests/comm_layout_dump.cpp prints it on the CPU and tests/test_gather_layout.py holds it to
// tests/gather_reference.py.
//
//   rank r's slab, slab_bytes long, at byte r * slab_bytes of the gathered buffer:
//     [ 8 rows x 8 n_r columns x 3 elements: its tiles side by side (rt_render's tile_shard layout) |
//       padding up to slab_elems = 192 n_max elements, never written                                |
//       status: int32 0, or -rc of a shard render that failed; int32 0 ]
//   n_max is rank 0's tile count, the largest. The 8 trailer bytes keep slab_bytes a multiple of
//   the element size, so the kernel's stride is a whole number of elements: 192 n_max + 1 in f64,
//   192 n_max + 2 in f32.
#pragma once

#include <cstddef>
#include <cstdint>

#include "launch_plan.hpp"

namespace rtc {

constexpr size_t kTrailerBytes = 8;   // the status word and its padding, sent with the slab
constexpr long long kTileElems = 8 * 8 * 3;   // one 8x8 tile's elements

struct SlabLayout {
    int world = 1;
    int n_max = 0, n_mine = 0;   // tiles of the largest shard (rank 0's), and of this rank's
    size_t esz = 8;              // bytes per element: 8 (RT_OUT_F64) or 4 (RT_OUT_F32)
    long long slab_elems = 0;    // 8 x 8 n_max x 3: the tile part of a slab
    size_t slab_bytes = 0;       // what every rank sends, and the bytes per rank in the gathered buffer

    size_t status_off() const { return (size_t)slab_elems * esz; }                    // the trailer, within a slab
    size_t status_at(int r) const { return (size_t)r * slab_bytes + status_off(); }   // rank r's, in the gathered buffer
    size_t gathered_bytes() const { return slab_bytes * (size_t)world; }
    long long stride_elems() const { return (long long)(slab_bytes / esz); }          // assemble_tiles' slab_elems
};

// The layout of a width x height frame's slabs on `rank` of `world`; n_max 0 when the frame has
// too many tiles for a tile shard (rtp::tiles_in_shard).
inline SlabLayout slab_layout(int width, int height, int rank, int world, size_t esz)
{
    SlabLayout l;
    l.world = world;
    l.esz = esz;
    l.n_max = rtp::tiles_in_shard(width, height, 0, world);
    l.n_mine = rtp::tiles_in_shard(width, height, rank, world);
    l.slab_elems = kTileElems * l.n_max;
    l.slab_bytes = (size_t)l.slab_elems * esz + kTrailerBytes;
    return l;
}

// The trailer a rank writes after its shard render returned rc (RT_OK or an RT_ERR_*).
inline int32_t status_of(int rc) { return rc ? -rc : 0; }

struct StatusScan {
    int failed = 0;     // ranks whose status is not 0
    int first = -1;     // the lowest of them (-1: none)
    int first_rc = 0;   // and the rc its render returned
};

inline StatusScan scan_status(const int32_t* status, int world)
{
    StatusScan s;
    for (int r = 0; r < world; ++r) {
        if (status[r] == 0) continue;
        if (s.failed++ == 0) {
            s.first = r;
            s.first_rc = -status[r];
        }
    }
    return s;
}

}  // namespace rtc
