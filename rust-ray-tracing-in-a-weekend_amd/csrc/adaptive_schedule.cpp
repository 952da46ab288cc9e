// adaptive_schedule.cpp — see adaptive_schedule.hpp
#include "adaptive_schedule.hpp"

#include <algorithm>
#include <cmath>

namespace rtas {

// v rounded up to a multiple of c (c >= 1), not clamped
static long long round_up_ll(long long v, long long c) { return (v + c - 1) / c * c; }

int round_up(int v, int chunk)
{
    const long long c = std::max(chunk, 1);
    return (int)std::min<long long>(round_up_ll(v, c), 0x7fffffffLL / c * c);
}

int next_count(int64_t n, int cap, int min_r, int step_r)
{
    return (int)std::min<int64_t>(cap, n == 0 ? (int64_t)min_r : n + (int64_t)step_r);
}

// what create and the one-shot call share: a whole frame, its geometry, ap's bounds
static const char* check_frame(const rt_render_params* p, const rt_adaptive_params* ap)
{
    if (p->row_begin != 0 || (p->row_stride != 0 && p->row_stride != 1) || p->row_block < 0 || p->row_block > 1 ||
        p->tile_shard != 0)
        return "adaptive sampling renders whole frames: the shard fields must be unset";
    if (p->width < 2 || p->height < 2 || (long long)p->width * p->height > 0xffffffffLL || p->spp_chunk < 0 ||
        p->max_depth < 0)
        return "bad render params";
    if ((long long)((p->width + 7) / 8) * ((p->height + 7) / 8) > 0x3fffffffLL) return "too many tiles";
    if (ap->min_spp < 2 || ap->step_spp < 1) return "bad adaptive params (min_spp >= 2, step_spp >= 1)";
    return nullptr;
}

const char* check_create(const rt_render_params* p, const rt_adaptive_params* ap, int auto_chunk, Schedule& s)
{
    if (const char* msg = check_frame(p, ap)) return msg;
    if (p->spp_chunk == 0 && p->spp < 1) return "bad render params";
    s.chunk = p->spp_chunk > 0 ? p->spp_chunk : std::max(auto_chunk, 1);
    if (ap->min_spp > 0x40000000 || ap->step_spp > 0x40000000 || s.chunk > 0x40000000)
        return "bad adaptive params (min_spp, step_spp and the chunk are at most 2^30)";
    s.min_r = round_up(ap->min_spp, s.chunk);
    s.step_r = round_up(ap->step_spp, s.chunk);
    return nullptr;
}

const char* check_one_shot(const rt_render_params* p, const rt_adaptive_params* ap, int auto_chunk, Schedule& s)
{
    if (const char* msg = check_frame(p, ap)) return msg;
    if (p->spp < 2 || (p->out_format != RT_OUT_F32 && p->out_format != RT_OUT_F64))
        return "bad render params (adaptive sampling needs spp >= 2)";
    if (std::isnan(ap->threshold)) return "bad adaptive params (threshold not NaN)";
    s.chunk = p->spp_chunk > 0 ? std::min(p->spp_chunk, p->spp) : std::max(auto_chunk, 1);
    s.min_r = (int)std::min<long long>(p->spp, round_up_ll(ap->min_spp, s.chunk));
    s.step_r = (int)std::min<long long>(p->spp, round_up_ll(ap->step_spp, s.chunk));
    return nullptr;
}

const char* check_advance(const rt_adaptive_advance_params* a, int ragged_cap, bool any_zero)
{
    if (std::isnan(a->threshold)) return "rt_adaptive_state_advance: the threshold is NaN";
    if (a->spp_cap < 2) return "rt_adaptive_state_advance: spp_cap < 2";
    if (a->max_launches < 0) return "rt_adaptive_state_advance: max_launches < 0";
    if (ragged_cap > 0 && a->spp_cap > ragged_cap)
        return "rt_adaptive_state_advance: an earlier cap closed a partial chunk; a larger cap would split its sum";
    if (a->tile_error_in) {
        if (a->max_launches != 0) return "rt_adaptive_state_advance: a caller's error map is one round (max_launches must be 0)";
        if (any_zero) return "rt_adaptive_state_advance: a caller's error map needs every tile past its first samples";
    }
    return nullptr;
}

int ragged_after(int ragged_cap, int end, int chunk) { return end % std::max(chunk, 1) != 0 ? end : ragged_cap; }

const char* check_restore(const rt_adaptive_state_header* h, const uint32_t* tile_spp, int64_t n_tiles, int width,
                          int height, const Schedule& s, bool with_halves)
{
    if (h->width != width || h->height != height) return "rt_adaptive_state_set: another frame size";
    if (h->spp_chunk != s.chunk || h->min_spp != s.min_r || h->step_spp != s.step_r)
        return "rt_adaptive_state_set: another chunk, min_spp or step_spp";
    if ((h->with_halves != 0) != with_halves) return "rt_adaptive_state_set: with_halves differs";
    if (h->ragged_cap < 0 || (h->ragged_cap > 0 && h->ragged_cap % s.chunk == 0))
        return "rt_adaptive_state_set: bad ragged_cap";
    for (int64_t t = 0; t < n_tiles; ++t) {
        const uint32_t n = tile_spp[t];
        if (n == 1 || n > 0x7fffffffu) return "rt_adaptive_state_set: a tile count of 1, or past 2^31 - 1";
        if (n % (uint32_t)s.chunk != 0 && (int64_t)n != (int64_t)h->ragged_cap)
            return "rt_adaptive_state_set: a tile count off the chunk grid that is not the ragged cap";
    }
    return nullptr;
}

rt_adaptive_group next_group(const uint32_t* tile_spp, const double* tile_error, const uint8_t* selected,
                             int64_t n_tiles, double threshold, int cap, int min_r, int step_r, uint32_t* group_out)
{
    auto is_active = [&](int64_t t) {
        return selected ? (selected[t] != 0 && tile_spp[t] < (uint32_t)cap)
                        : active(tile_spp[t], tile_error[t], threshold, cap);
    };
    rt_adaptive_group g{};
    uint32_t lowest = 0xffffffffu;
    for (int64_t t = 0; t < n_tiles; ++t) {
        if (!is_active(t)) continue;
        g.n_active += 1;
        lowest = std::min(lowest, tile_spp[t]);
    }
    if (g.n_active == 0) return g;
    for (int64_t t = 0; t < n_tiles; ++t) {
        if (!is_active(t) || tile_spp[t] != lowest) continue;
        if (group_out) group_out[g.n_group] = (uint32_t)t;
        g.n_group += 1;
    }
    g.n_star = (int32_t)lowest;
    g.n_next = next_count(lowest, cap, min_r, step_r);
    return g;
}

}  // namespace rtas
