// deal_cache.cpp — see deal_cache.hpp.
#include "deal_cache.hpp"

#include <algorithm>
#include <cstring>
#include <numeric>

namespace rtd {

Key key_of(uint64_t upload_gen, const rt_camera& cam, const rt_render_params& p)
{
    Key k;
    k.upload_gen = upload_gen;
    k.cam = cam;
    k.width = p.width;
    k.height = p.height;
    k.row_begin = p.row_begin;
    k.row_stride = p.row_stride;
    k.row_block = p.row_block > 1 ? p.row_block : 1;
    return k;
}

bool same_key(const Key& a, const Key& b)
{
    // (rt_camera is doubles only: no padding; the bytes, so a NaN camera still equals itself)
    return a.upload_gen == b.upload_gen && std::memcmp(&a.cam, &b.cam, sizeof a.cam) == 0 && a.width == b.width &&
           a.height == b.height && a.row_begin == b.row_begin && a.row_stride == b.row_stride &&
           a.row_block == b.row_block;
}

bool eligible(const rt_render_params& p, int schedule, bool adaptive_pass)
{
    return !p.tile_shard && p.row_begin == 0 && p.row_stride == 1 && !p.count_work && !adaptive_pass &&
           (schedule == RT_SCHED_POOL || schedule == RT_SCHED_ITEMS);
}

Decision DealCache::next(int mode, bool is_eligible, const Key& k, int64_t n_tiles)
{
    Decision d;
    if (!is_eligible || mode == kOff || n_tiles <= 0) return d;
    const bool hit = state_ != kEmpty && n_tiles_ == n_tiles && same_key(key_, k);
    if (mode == kMeasureOnly || !hit) {   // a new key's first render, or every render of the A/B mode
        drop();
        state_ = kMeasured;
        key_ = k;
        n_tiles_ = n_tiles;
        d.measure = true;
        return d;
    }
    d.build = state_ == kMeasured;   // (finish_build makes it kOrdered)
    d.ordered = true;
    return d;
}

const std::vector<uint32_t>& DealCache::finish_build(const uint64_t* costs)
{
    order_.resize((size_t)n_tiles_);
    cost_order(costs, n_tiles_, order_.data());
    state_ = kOrdered;
    return order_;
}

void DealCache::drop()
{
    state_ = kEmpty;
    n_tiles_ = 0;
    order_.clear();
}

void cost_order(const uint64_t* costs, int64_t n, uint32_t* order)
{
    std::iota(order, order + n, 0u);
    std::stable_sort(order, order + n, [costs](uint32_t a, uint32_t b) { return costs[a] > costs[b]; });
}

}  // namespace rtd
