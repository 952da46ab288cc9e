// abi_adaptive_state.cpp — rt_adaptive_state behind the C ABI (include/rt/rt_abi.h): an adaptive
// frame's device side (adaptive_frame.hpp) owned between calls, with the camera, the launch params
// and the schedule it was created with. Every check made here is adaptive_schedule.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>

#include "rt/rt_abi.h"
#include "adaptive_frame.hpp"
#include "ctx_internal.hpp"
#include "render_internal.hpp"

struct rt_adaptive_state {
    rt_ctx* ctx = nullptr;
    rt_camera cam{};
    rt_render_params rp{};           // a launch: the tail of the state's tile order as one tile shard
    uint64_t upload_gen = 0;         // the context's scene upload the state is bound to
    rtas::Schedule sched;
    AdaptiveBlock fr;
    DevBuf stage;                    // resolve's staging of host-bound outputs
    rt_adaptive_state_stats stats{};
};

namespace {

// tile_spp's range on the host (a restored checkpoint)
void count_range(const uint32_t* tile_spp, int n_tiles, uint32_t& lo, uint32_t& hi)
{
    lo = 0xffffffffu, hi = 0;
    for (int t = 0; t < n_tiles; ++t) {
        lo = std::min(lo, tile_spp[t]);
        hi = std::max(hi, tile_spp[t]);
    }
}

// A checkpoint's arrays, to the host or from it: the sizes and the device pointers are the block's
int copy_checkpoint(const AdaptiveBlock& fr, const rt_adaptive_state_data* data, bool to_host)
{
    const size_t hw = (size_t)fr.width * (size_t)fr.height, nt = (size_t)fr.n_tiles;
    auto copy = [&](void* host, void* dev, size_t bytes) {
        return to_host ? hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) : hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice);
    };
    HIP_TRY(copy(data->sums, fr.F.sum, 3 * hw * sizeof(double)));
    HIP_TRY(copy(data->q, fr.F.q, hw * sizeof(double)));
    HIP_TRY(copy(data->tile_spp, fr.F.tile_spp, nt * sizeof(uint32_t)));
    HIP_TRY(copy(data->tile_error, fr.F.tile_error, nt * sizeof(double)));
    if (fr.with_halves) {
        HIP_TRY(copy(data->sum_a, fr.Hf.sum_a, 3 * hw * sizeof(double)));
        HIP_TRY(copy(data->sum_b, fr.Hf.sum_b, 3 * hw * sizeof(double)));
    }
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_adaptive_next_group_host(const uint32_t* tile_spp, const double* tile_error, const uint8_t* selected,
                                int64_t n_tiles, double threshold, int32_t spp_cap, int32_t min_r, int32_t step_r,
                                uint32_t* group_out, rt_adaptive_group* out)
{
    if (!tile_spp || !out) return fail(RT_ERR_INVALID, "null argument");
    if ((tile_error != nullptr) == (selected != nullptr))
        return fail(RT_ERR_INVALID, "rt_adaptive_next_group_host: give tile_error or selected, not both");
    if (n_tiles < 1 || n_tiles > 0x3fffffffLL || spp_cap < 2 || min_r < 2 || step_r < 1 || std::isnan(threshold))
        return fail(RT_ERR_INVALID, "rt_adaptive_next_group_host: bad tile count, cap, min, step or threshold");
    *out = rtas::next_group(tile_spp, tile_error, selected, n_tiles, threshold, spp_cap, min_r, step_r, group_out);
    return RT_OK;
}

int rt_adaptive_state_create(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_adaptive_params* ap,
                             int with_halves, rt_adaptive_state** out)
{
    if (!c || !cam || !p || !ap || !out) return fail(RT_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!c->has_scene) return fail(RT_ERR_NO_SCENE, "no scene uploaded");
    rtas::Schedule sched;
    if (const char* msg = rtas::check_create(p, ap, auto_chunk(std::max(p->spp, 1)), sched)) return fail(RT_ERR_INVALID, msg);
    if (c->opt.precision == RT_PREC_F32) return fail(RT_ERR_UNSUPPORTED, "adaptive sampling in the f32 mode");

    auto* st = new (std::nothrow) rt_adaptive_state;
    if (!st) return fail(RT_ERR_OOM, "out of host memory");
    st->ctx = c;
    st->cam = *cam;
    st->rp = *p;
    st->rp.row_stride = 1;
    st->rp.row_block = 0;
    st->rp.tile_shard = 1;
    st->rp.count_work = 0;
    st->rp.out_on_device = 0;
    st->upload_gen = c->upload_gen;
    st->sched = sched;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = st->fr.init(p->width, p->height, with_halves != 0, nullptr);
    if (e != hipSuccess) {
        delete st;
        return hip_fail(e, "rt_adaptive_state_create");
    }
    st->stats.spp_chunk = sched.chunk;
    st->stats.min_spp = sched.min_r;
    st->stats.step_spp = sched.step_r;
    st->stats.tiles = st->fr.n_tiles;
    st->stats.active_left = st->fr.n_tiles;
    *out = st;
    return RT_OK;
}

void rt_adaptive_state_destroy(rt_adaptive_state* st)
{
    if (!st) return;
    (void)hipSetDevice(st->ctx->device);
    (void)hipDeviceSynchronize();   // (every call on a state ends synchronized: nothing reads its buffers)
    delete st;
}

int rt_adaptive_state_advance(rt_adaptive_state* st, const rt_adaptive_advance_params* ap, int32_t* active_left)
{
    if (!st || !ap) return fail(RT_ERR_INVALID, "null argument");
    rt_ctx* c = st->ctx;
    if (c->opt.precision == RT_PREC_F32) return fail(RT_ERR_UNSUPPORTED, "adaptive sampling in the f32 mode");
    if (!c->has_scene) return fail(RT_ERR_NO_SCENE, "no scene uploaded");
    if (c->upload_gen != st->upload_gen)
        return fail(RT_ERR_INVALID, "rt_adaptive_state_advance: the context's scene was uploaded again after the state was created");
    if (const char* msg = rtas::check_advance(ap, st->fr.ragged_cap, st->fr.min_count == 0)) return fail(RT_ERR_INVALID, msg);

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = ap->stream ? (hipStream_t)ap->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;

    AdaptiveAdvance adv;
    rc = st->fr.advance(c, &st->cam, st->rp, st->sched, ap->threshold, ap->spp_cap, ap->max_launches, ap->tile_error_in,
                        ap->error_on_device != 0, stream, adv);
    rt_adaptive_state_stats& s = st->stats;   // (what was launched counts, also when a later launch failed)
    s.groups = adv.launches;
    s.samples_traced = adv.samples;
    s.trace_ms = adv.trace_ms;
    s.moments_ms = adv.moments_ms;
    s.classify_ms = adv.classify_ms;
    s.groups_total += adv.launches;
    s.samples_total += adv.samples;
    if (rc) return rc;
    s.active_left = adv.active_left;
    s.min_count = (int32_t)st->fr.min_count;
    s.max_count = (int32_t)st->fr.max_count;
    if (active_left) *active_left = adv.active_left;
    rc = scope.end();
    if (rc) return rc;
    adaptive_last_stats(c, adv, ap->spp_cap, st->sched.chunk, st->fr.n_tiles);
    return RT_OK;
}

int rt_adaptive_state_resolve(rt_adaptive_state* st, int out_format, int on_device, const rt_adaptive_out* out,
                              const rt_adaptive_halves* hv)
{
    if (!st || !out || !out->mean) return fail(RT_ERR_INVALID, "null argument");
    if (out_format != RT_OUT_F32 && out_format != RT_OUT_F64) return fail(RT_ERR_INVALID, "bad out_format");
    if (hv) {
        if (!st->fr.with_halves) return fail(RT_ERR_INVALID, "rt_adaptive_state_resolve: the state was created without halves");
        if (!hv->mean_a || !hv->mean_b) return fail(RT_ERR_INVALID, "null argument");
        if (hv->mean_a == hv->mean_b || hv->mean_a == out->mean || hv->mean_b == out->mean)
            return fail(RT_ERR_INVALID, "rt_adaptive_halves: mean_a, mean_b and the mean must be three buffers");
    }
    if (st->fr.min_count == 0) return fail(RT_ERR_INVALID, "rt_adaptive_state_resolve: a tile has no samples yet");
    rt_ctx* c = st->ctx;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;
    rc = st->fr.resolve(out_format, on_device != 0, out, hv, st->stage, stream);
    if (rc) return rc;
    rc = scope.end();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

int rt_adaptive_state_get(rt_adaptive_state* st, rt_adaptive_state_header* header, const rt_adaptive_state_data* data)
{
    if (!st || !header) return fail(RT_ERR_INVALID, "null argument");
    if (data && (!data->sums || !data->q || !data->tile_spp || !data->tile_error ||
                 (st->fr.with_halves && (!data->sum_a || !data->sum_b))))
        return fail(RT_ERR_INVALID, "rt_adaptive_state_data: a null array");
    *header = rt_adaptive_state_header{};
    header->width = st->fr.width;
    header->height = st->fr.height;
    header->spp_chunk = st->sched.chunk;
    header->min_spp = st->sched.min_r;
    header->step_spp = st->sched.step_r;
    header->with_halves = st->fr.with_halves ? 1 : 0;
    header->ragged_cap = st->fr.ragged_cap;
    header->groups_total = st->stats.groups_total;
    header->samples_total = st->stats.samples_total;
    if (!data) return RT_OK;
    HIP_TRY(hipSetDevice(st->ctx->device));
    return copy_checkpoint(st->fr, data, true);
}

int rt_adaptive_state_set(rt_adaptive_state* st, const rt_adaptive_state_header* header, const rt_adaptive_state_data* data)
{
    if (!st || !header || !data) return fail(RT_ERR_INVALID, "null argument");
    AdaptiveBlock& fr = st->fr;
    if (!data->sums || !data->q || !data->tile_spp || !data->tile_error || (fr.with_halves && (!data->sum_a || !data->sum_b)))
        return fail(RT_ERR_INVALID, "rt_adaptive_state_data: a null array");
    if (const char* msg = rtas::check_restore(header, data->tile_spp, fr.n_tiles, fr.width, fr.height, st->sched, fr.with_halves))
        return fail(RT_ERR_INVALID, msg);
    HIP_TRY(hipSetDevice(st->ctx->device));
    const int rc = copy_checkpoint(fr, data, false);
    if (rc) return rc;
    fr.ragged_cap = header->ragged_cap;
    count_range(data->tile_spp, fr.n_tiles, fr.min_count, fr.max_count);
    st->stats.groups_total = header->groups_total;
    st->stats.samples_total = header->samples_total;
    st->stats.min_count = (int32_t)fr.min_count;
    st->stats.max_count = (int32_t)fr.max_count;
    return RT_OK;
}

int rt_adaptive_state_last_stats(rt_adaptive_state* st, rt_adaptive_state_stats* out)
{
    if (!st || !out) return fail(RT_ERR_INVALID, "null argument");
    *out = st->stats;
    return RT_OK;
}

}  // extern "C"
