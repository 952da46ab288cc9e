// deal_cache.hpp — the order a context deals a whole frame's work blocks in, measured by the
// product render itself and kept per (scene upload, camera, frame). A launch ends on its longest
// paths; dealt most expensive tiles first, all of a tile's sample groups together, it ends on the
// cheap tiles instead. The first eligible render of a key runs in raster order
// and has the pool kernel add each wave's cycles between block fetches to the block's tile
// (KParams.deal_cost); the second reads those costs back once, sorts them and uploads the order
// (KParams.deal_order); every later one reuses it. Pure state and arithmetic, no HIP and no
// context: abi.cpp's run_range allocates, copies and enqueues what next() decides;
// tests/deal_cache_main.cpp runs it on a CPU.
#pragma once

#include <cstdint>
#include <vector>

#include "rt/rt_abi.h"

namespace rtd {

// RT_OPT_AUTO_DEAL_ORDER
enum Mode { kOff = 0, kAuto = 1, kMeasureOnly = 2 };

// What an order belongs to. Not the spp, seed, depth or sample range: a tile's relative cost
// does not depend on them.
struct Key {
    uint64_t upload_gen = 0;    // the context's scene upload (counted from 1)
    rt_camera cam{};
    int32_t width = 0, height = 0;
    int32_t row_begin = 0, row_stride = 1, row_block = 1;   // the row-shard geometry
};
Key key_of(uint64_t upload_gen, const rt_camera& cam, const rt_render_params& p);
bool same_key(const Key& a, const Key& b);

// A render takes part when it is a whole frame (no tile shard, every row) on a pool schedule
// (schedule: RT_SCHED_*, AUTO resolved), not a count_work render and not an rt_render_adaptive
// pass (which deals its own order).
bool eligible(const rt_render_params& p, int schedule, bool adaptive_pass);

struct Decision {
    bool measure = false;   // zero the tile costs, then launch with KParams.deal_cost
    bool build = false;     // first read the costs back, build the order (finish_build) and upload it
    bool ordered = false;   // launch with KParams.deal_order (tile-major)
};

class DealCache {
public:
    // What the next render does; one call per render, before its launches. An ineligible render
    // or mode kOff decides nothing and leaves the entry as it is.
    Decision next(int mode, bool is_eligible, const Key& k, int64_t n_tiles);
    // after a `build` decision: the order from the costs read back; fail_build() if that failed
    // (the entry is dropped, the render runs in raster order)
    const std::vector<uint32_t>& finish_build(const uint64_t* costs);
    void fail_build() { drop(); }
    // a new upload, or the context's end
    void drop();

    enum State { kEmpty, kMeasured, kOrdered };
    State state() const { return state_; }
    int64_t n_tiles() const { return n_tiles_; }
    const std::vector<uint32_t>& order() const { return order_; }   // kOrdered: position -> raster tile

private:
    State state_ = kEmpty;
    Key key_;
    int64_t n_tiles_ = 0;
    std::vector<uint32_t> order_;
};

// Raster tiles sorted by cost, most expensive first, ties (and so tiles with no measured block,
// cost 0, at the end) in raster order: rt_cost_tile_order.
void cost_order(const uint64_t* costs, int64_t n, uint32_t* order);

}  // namespace rtd
