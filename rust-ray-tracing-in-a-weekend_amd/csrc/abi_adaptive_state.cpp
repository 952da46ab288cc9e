// abi_adaptive_state.cpp — rt_adaptive_state behind the C ABI (include/rt/rt_abi.h): the adaptive
// frame's accumulators owned between calls and advanced by rt_render_adaptive's trace passes and
// moments kernel (run_range with the moments sink, render_internal.hpp). What a launch traces is
// chosen on the device (adaptive_state_kernel.hip) by the rule of adaptive_schedule.hpp, which also
// holds every check made here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <vector>

#include "rt/rt_abi.h"
#include "adaptive_schedule.hpp"
#include "adaptive_state_kernel.hpp"
#include "ctx_internal.hpp"
#include "render_internal.hpp"

// What render_adaptive keeps in its call-local block, owned: one allocation,
// [sum | sum_open | q | q_open | tile_error | a caller's map | halves: sum_a | sum_a_open | sum_b |
// sum_b_open] f64, then [tile_spp | order | mask | the regroup record] u32; zeroed at create.
struct rt_adaptive_state {
    rt_ctx* ctx = nullptr;
    rt_camera cam{};
    rt_render_params rp{};           // a launch: the tail of the state's tile order as one tile shard
    uint64_t upload_gen = 0;         // the context's scene upload the state is bound to
    int width = 0, height = 0, n_tiles = 0;
    rtas::Schedule sched;
    bool with_halves = false;
    DevBuf blk;
    rtk::AdaptiveFrame F{};
    rtk::AdaptiveHalves Hf{};
    uint32_t* order = nullptr;       // [every other tile | the group]
    uint32_t* mask = nullptr;        // a caller's-map round: the tiles still to step
    double* error_in = nullptr;      //   its map, when the caller's is on the host
    rtk::RegroupRecord* record = nullptr;
    bool order_is_raster = true;     // no regroup has run: the order is the one create wrote
    DevBuf stage;                    // resolve's staging of host-bound outputs
    EventSpan<2> ev;                 // around a group's regroup and its readback
    // the host side
    int ragged_cap = 0;              // 0, or the cap at which a launch closed a partial chunk
    uint32_t min_count = 0, max_count = 0;
    rt_adaptive_state_stats stats{};
};

namespace {

size_t frame_px(const rt_adaptive_state* st) { return (size_t)st->width * (size_t)st->height; }

// tile_spp's range on the host (a restored checkpoint)
void count_range(const uint32_t* tile_spp, int n_tiles, uint32_t& lo, uint32_t& hi)
{
    lo = 0xffffffffu, hi = 0;
    for (int t = 0; t < n_tiles; ++t) {
        lo = std::min(lo, tile_spp[t]);
        hi = std::max(hi, tile_spp[t]);
    }
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
    rt_render_params rp = *p;
    rp.row_stride = 1;
    rp.row_block = 0;
    rp.tile_shard = 1;
    rp.count_work = 0;
    rp.out_on_device = 0;
    rp.stream = nullptr;
    if (bad_geometry(&rp)) return fail(RT_ERR_INVALID, "bad render params");

    auto* st = new (std::nothrow) rt_adaptive_state;
    if (!st) return fail(RT_ERR_OOM, "out of host memory");
    st->ctx = c;
    st->cam = *cam;
    st->rp = rp;
    st->upload_gen = c->upload_gen;
    st->width = p->width;
    st->height = p->height;
    st->n_tiles = ((p->width + 7) / 8) * ((p->height + 7) / 8);
    st->sched = sched;
    st->with_halves = with_halves != 0;

    const size_t hw = frame_px(st), nt = (size_t)st->n_tiles;
    const size_t n_f64 = 8 * hw + 2 * nt + (st->with_halves ? 12 * hw : 0);
    const size_t n_u32 = 3 * nt + sizeof(rtk::RegroupRecord) / sizeof(uint32_t);
    const size_t bytes = n_f64 * sizeof(double) + n_u32 * sizeof(uint32_t);
    std::vector<uint32_t> raster(nt);
    for (size_t i = 0; i < nt; ++i) raster[i] = (uint32_t)i;
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = st->blk.alloc(bytes);
    if (e == hipSuccess) e = hipMemset(st->blk.p, 0, bytes);
    double* d = st->blk.as<double>();
    uint32_t* u = (uint32_t*)(d + n_f64);
    if (e == hipSuccess) e = hipMemcpy(u + nt, raster.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = st->ev.create();
    if (e != hipSuccess) {
        delete st;
        return hip_fail(e, "rt_adaptive_state_create");
    }
    st->F.sum = d;
    st->F.sum_open = d + 3 * hw;
    st->F.q = d + 6 * hw;
    st->F.q_open = d + 7 * hw;
    st->F.tile_error = d + 8 * hw;
    st->error_in = d + 8 * hw + nt;
    if (st->with_halves) {
        double* h = d + 8 * hw + 2 * nt;
        st->Hf.sum_a = h;
        st->Hf.sum_a_open = h + 3 * hw;
        st->Hf.sum_b = h + 6 * hw;
        st->Hf.sum_b_open = h + 9 * hw;
    }
    st->F.tile_spp = u;
    st->order = u + nt;
    st->mask = u + 2 * nt;
    st->record = (rtk::RegroupRecord*)(u + 3 * nt);
    st->F.order = st->order;
    st->F.width = st->width;
    st->F.height = st->height;
    st->F.tiles_x = (st->width + 7) / 8;
    st->stats.spp_chunk = sched.chunk;
    st->stats.min_spp = sched.min_r;
    st->stats.step_spp = sched.step_r;
    st->stats.tiles = st->n_tiles;
    st->stats.active_left = st->n_tiles;
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
    if (const char* msg = rtas::check_advance(ap, st->ragged_cap, st->min_count == 0)) return fail(RT_ERR_INVALID, msg);
    const int n_tiles = st->n_tiles, chunk = st->sched.chunk, cap = ap->spp_cap;
    const bool by_map = ap->tile_error_in != nullptr;

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = ap->stream ? (hipStream_t)ap->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;

    st->stats.groups = 0;
    st->stats.samples_traced = 0;
    st->stats.trace_ms = st->stats.moments_ms = st->stats.classify_ms = 0.0;
    uint32_t* const mask = by_map ? st->mask : nullptr;
    if (by_map) {   // the selected set, fixed here
        const double* map = ap->tile_error_in;
        if (!ap->error_on_device) {
            HIP_TRY(hipMemcpyAsync(st->error_in, map, (size_t)n_tiles * sizeof(double), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));   // (the caller's array is read until the copy is done)
            map = st->error_in;
        }
        HIP_TRY(rtk::launch_adaptive_select_mask(st->F.tile_spp, map, mask, n_tiles, ap->threshold, (uint32_t)cap, stream));
    }

    // a regroup and its record: one synchronization
    rtk::RegroupRecord rec{};
    auto regroup = [&]() -> int {
        HIP_TRY(st->ev.record(0, stream));
        HIP_TRY(rtk::launch_adaptive_regroup(st->F.tile_spp, st->F.tile_error, mask, st->order, n_tiles, ap->threshold,
                                             (uint32_t)cap, st->record, stream));
        HIP_TRY(hipMemcpyAsync(&rec, st->record, sizeof rec, hipMemcpyDeviceToHost, stream));
        HIP_TRY(st->ev.record(1, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float t_classify = 0;
        HIP_TRY(st->ev.elapsed(0, &t_classify));
        st->stats.classify_ms += t_classify;
        st->order_is_raster = false;
        if (rec.n_group > (uint32_t)n_tiles || rec.n_active > (uint32_t)n_tiles || rec.n_group > rec.n_active ||
            (rec.n_group > 0 && rec.n_star >= (uint32_t)cap))
            return fail(RT_ERR_HIP, "adaptive regroup: inconsistent record");
        st->min_count = rec.n_min;
        st->max_count = rec.n_max;
        return RT_OK;
    };
    if (!by_map && st->max_count == 0 && st->order_is_raster) {
        // a fresh state: every tile at 0, the group is the frame in the raster order create wrote
        rec.n_group = rec.n_active = (uint32_t)n_tiles;
    } else {
        rc = regroup();
        if (rc) return rc;
    }

    int batches = 0;
    while (rec.n_group > 0 && (ap->max_launches == 0 || st->stats.groups < ap->max_launches)) {
        const int first = (int)rec.n_star, end = rtas::next_count(first, cap, st->sched.min_r, st->sched.step_r);
        const int n_group = (int)rec.n_group;
        st->rp.row_begin = n_tiles - n_group;
        st->rp.spp = end;
        st->rp.stream = stream;
        st->F.pos_begin = n_tiles - n_group;
        Sink sink;
        sink.moments = &st->F;
        sink.n_done = end;
        sink.halves = st->with_halves ? &st->Hf : nullptr;
        rc = run_range(c, &st->cam, &st->rp, first, end, chunk, stream, sink);
        if (rc) return rc;
        st->ragged_cap = rtas::ragged_after(st->ragged_cap, end, chunk);
        const int trace_batches = c->stats.n_batches;
        rc = regroup();
        if (rc) return rc;
        float t_trace = 0, t_moments = 0;
        HIP_TRY(c->ev.elapsed(0, &t_trace));   // (the launch's render span, read here: disarmed below)
        HIP_TRY(c->ev.elapsed(1, &t_moments));
        const uint64_t samples = 64ull * (uint64_t)n_group * (uint64_t)(end - first);
        st->stats.trace_ms += t_trace;
        st->stats.moments_ms += t_moments;
        st->stats.groups += 1;
        st->stats.samples_traced += samples;
        st->stats.groups_total += 1;
        st->stats.samples_total += samples;
        batches += trace_batches;
    }
    st->stats.active_left = (int32_t)rec.n_active;
    st->stats.min_count = (int32_t)st->min_count;
    st->stats.max_count = (int32_t)st->max_count;
    if (active_left) *active_left = (int32_t)rec.n_active;
    rc = scope.end();
    if (rc) return rc;

    // rt_last_stats: the call as a whole, as rt_render_adaptive (the variant fields are the last launch's)
    c->stats.kernel_ms = st->stats.trace_ms;
    c->stats.reduce_ms = st->stats.moments_ms;
    c->stats.samples = st->stats.samples_traced;
    c->stats.n_batches = batches;
    c->stats.n_chunks = (cap + chunk - 1) / chunk;
    c->stats.n_items = 64ull * (uint64_t)n_tiles * (uint64_t)c->stats.n_chunks;
    c->stats.casts = c->stats.node_visits = c->stats.prim_tests = 0;
    c->ev.disarm();
    c->pending_counts = false;
    return RT_OK;
}

int rt_adaptive_state_resolve(rt_adaptive_state* st, int out_format, int on_device, const rt_adaptive_out* out,
                              const rt_adaptive_halves* hv)
{
    if (!st || !out || !out->mean) return fail(RT_ERR_INVALID, "null argument");
    if (out_format != RT_OUT_F32 && out_format != RT_OUT_F64) return fail(RT_ERR_INVALID, "bad out_format");
    if (hv) {
        if (!st->with_halves) return fail(RT_ERR_INVALID, "rt_adaptive_state_resolve: the state was created without halves");
        if (!hv->mean_a || !hv->mean_b) return fail(RT_ERR_INVALID, "null argument");
        if (hv->mean_a == hv->mean_b || hv->mean_a == out->mean || hv->mean_b == out->mean)
            return fail(RT_ERR_INVALID, "rt_adaptive_halves: mean_a, mean_b and the mean must be three buffers");
    }
    if (st->min_count == 0) return fail(RT_ERR_INVALID, "rt_adaptive_state_resolve: a tile has no samples yet");
    rt_ctx* c = st->ctx;
    const bool on_dev = on_device != 0, f64 = out_format == RT_OUT_F64;
    const size_t hw = frame_px(st), nt = (size_t)st->n_tiles;
    const size_t mean_bytes = hw * 3 * (f64 ? 8 : 4);

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;
    // host-bound outputs: staged [mean | mean_a | mean_b | se], a frame of f64 each at the most
    void *dev_mean = out->mean, *dev_a = hv ? hv->mean_a : nullptr, *dev_b = hv ? hv->mean_b : nullptr;
    double* dev_se = out->stderr_map;
    if (!on_dev) {
        rc = st->stage.reserve(stream, 10 * hw * sizeof(double));
        if (rc) return rc;
        double* s = st->stage.as<double>();
        dev_mean = s;
        dev_a = s + 3 * hw;
        dev_b = s + 6 * hw;
        dev_se = out->stderr_map ? s + 9 * hw : nullptr;
    }
    HIP_TRY(rtk::launch_adaptive_resolve(st->F.sum, st->F.q, st->F.tile_spp, dev_mean, f64, dev_se, st->width, st->height, stream));
    const hipMemcpyKind kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!on_dev) {
        HIP_TRY(hipMemcpyAsync(out->mean, dev_mean, mean_bytes, kind, stream));
        if (out->stderr_map) HIP_TRY(hipMemcpyAsync(out->stderr_map, dev_se, hw * sizeof(double), kind, stream));
    }
    if (out->tile_spp) HIP_TRY(hipMemcpyAsync(out->tile_spp, st->F.tile_spp, nt * sizeof(uint32_t), kind, stream));
    if (out->tile_error) HIP_TRY(hipMemcpyAsync(out->tile_error, st->F.tile_error, nt * sizeof(double), kind, stream));
    if (hv) {
        HIP_TRY(rtk::launch_adaptive_resolve_halves(st->Hf.sum_a, st->Hf.sum_b, st->F.tile_spp, dev_a, dev_b, f64, st->width,
                                                    st->height, stream));
        if (!on_dev) {
            HIP_TRY(hipMemcpyAsync(hv->mean_a, dev_a, mean_bytes, kind, stream));
            HIP_TRY(hipMemcpyAsync(hv->mean_b, dev_b, mean_bytes, kind, stream));
        }
    }
    rc = scope.end();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

int rt_adaptive_state_get(rt_adaptive_state* st, rt_adaptive_state_header* header, const rt_adaptive_state_data* data)
{
    if (!st || !header) return fail(RT_ERR_INVALID, "null argument");
    if (data && (!data->sums || !data->q || !data->tile_spp || !data->tile_error ||
                 (st->with_halves && (!data->sum_a || !data->sum_b))))
        return fail(RT_ERR_INVALID, "rt_adaptive_state_data: a null array");
    *header = rt_adaptive_state_header{};
    header->width = st->width;
    header->height = st->height;
    header->spp_chunk = st->sched.chunk;
    header->min_spp = st->sched.min_r;
    header->step_spp = st->sched.step_r;
    header->with_halves = st->with_halves ? 1 : 0;
    header->ragged_cap = st->ragged_cap;
    header->groups_total = st->stats.groups_total;
    header->samples_total = st->stats.samples_total;
    if (!data) return RT_OK;
    const size_t hw = frame_px(st), nt = (size_t)st->n_tiles;
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(hipMemcpy(data->sums, st->F.sum, 3 * hw * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(data->q, st->F.q, hw * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(data->tile_spp, st->F.tile_spp, nt * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(data->tile_error, st->F.tile_error, nt * sizeof(double), hipMemcpyDeviceToHost));
    if (st->with_halves) {
        HIP_TRY(hipMemcpy(data->sum_a, st->Hf.sum_a, 3 * hw * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(data->sum_b, st->Hf.sum_b, 3 * hw * sizeof(double), hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

int rt_adaptive_state_set(rt_adaptive_state* st, const rt_adaptive_state_header* header, const rt_adaptive_state_data* data)
{
    if (!st || !header || !data) return fail(RT_ERR_INVALID, "null argument");
    if (!data->sums || !data->q || !data->tile_spp || !data->tile_error || (st->with_halves && (!data->sum_a || !data->sum_b)))
        return fail(RT_ERR_INVALID, "rt_adaptive_state_data: a null array");
    if (const char* msg = rtas::check_restore(header, data->tile_spp, st->n_tiles, st->width, st->height, st->sched,
                                              st->with_halves))
        return fail(RT_ERR_INVALID, msg);
    const size_t hw = frame_px(st), nt = (size_t)st->n_tiles;
    HIP_TRY(hipSetDevice(st->ctx->device));
    HIP_TRY(hipMemcpy(st->F.sum, data->sums, 3 * hw * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st->F.q, data->q, hw * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st->F.tile_spp, data->tile_spp, nt * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(st->F.tile_error, data->tile_error, nt * sizeof(double), hipMemcpyHostToDevice));
    if (st->with_halves) {
        HIP_TRY(hipMemcpy(st->Hf.sum_a, data->sum_a, 3 * hw * sizeof(double), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(st->Hf.sum_b, data->sum_b, 3 * hw * sizeof(double), hipMemcpyHostToDevice));
    }
    st->ragged_cap = header->ragged_cap;
    count_range(data->tile_spp, st->n_tiles, st->min_count, st->max_count);
    st->stats.groups_total = header->groups_total;
    st->stats.samples_total = header->samples_total;
    st->stats.min_count = (int32_t)st->min_count;
    st->stats.max_count = (int32_t)st->max_count;
    return RT_OK;
}

int rt_adaptive_state_last_stats(rt_adaptive_state* st, rt_adaptive_state_stats* out)
{
    if (!st || !out) return fail(RT_ERR_INVALID, "null argument");
    *out = st->stats;
    return RT_OK;
}

}  // extern "C"
