// abi_passes.cpp — the auxiliary passes behind the C ABI (include/rt/rt_abi.h) that render through
// the driver (render_internal.hpp): tile-adaptive sampling, the first-hit feature buffers and the
// ray queries, with their stats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "rt/rt_abi.h"
#include "adaptive_criterion.hpp"
#include "adaptive_frame.hpp"
#include "ctx_internal.hpp"
#include "features_kernel.hpp"
#include "query_kernel.hpp"
#include "render_internal.hpp"

extern "C" {

// ---- tile-adaptive sampling (rt_abi.h: the criterion; adaptive_kernel.hip: the kernels) ----------
int rt_adaptive_tile_errors_host(const double* sums, const double* q, const uint32_t* tile_spp, int width,
                                 int height, double* tile_error_out, double* stderr_out)
{
    if (!sums || !q || !tile_spp) return fail(RT_ERR_INVALID, "null argument");
    if (width < 1 || height < 1 || (long long)width * height > 0xffffffffLL) return fail(RT_ERR_INVALID, "bad frame size");
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    for (long long t = 0; t < (long long)tiles_x * tiles_y; ++t)
        if (tile_spp[t] < 2) return fail(RT_ERR_INVALID, "a tile with fewer than 2 samples has no variance estimate");
    for (int ty = 0; ty < tiles_y; ++ty) {
        for (int tx = 0; tx < tiles_x; ++tx) {
            const size_t t = (size_t)ty * tiles_x + tx;
            const double n = (double)tile_spp[t];
            const int cw = std::min(8, width - tx * 8), ch = std::min(8, height - ty * 8);
            double e = 0.0;
            for (int k = 0; k < ch; ++k) {
                for (int i = 0; i < cw; ++i) {
                    const size_t px = (size_t)(ty * 8 + k) * width + (size_t)(tx * 8 + i);
                    const rtk::PixelNoise pn = rtk::adaptive_pixel_noise(sums[3 * px], sums[3 * px + 1], sums[3 * px + 2],
                                                                         q[px], n);
                    e = e + pn.e;
                    if (stderr_out) stderr_out[px] = pn.se;
                }
            }
            if (tile_error_out) tile_error_out[t] = e / (double)(cw * ch);
        }
    }
    return RT_OK;
}

}  // extern "C"

// rt_render_adaptive (hv null) and rt_render_adaptive_halves: a call-local frame (adaptive_frame.hpp)
// advanced to (ap->threshold, p->spp) and resolved, all on the call's stream
static int render_adaptive(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_adaptive_params* ap,
                           const rt_adaptive_out* out, const rt_adaptive_halves* hv)
{
    if (!c || !cam || !p || !ap || !out || !out->mean) return fail(RT_ERR_INVALID, "null argument");
    if (!c->has_scene) return fail(RT_ERR_NO_SCENE, "no scene uploaded");
    rtas::Schedule sched;
    if (const char* msg = rtas::check_one_shot(p, ap, auto_chunk(p->spp), sched)) return fail(RT_ERR_INVALID, msg);
    if (c->opt.precision == RT_PREC_F32) return fail(RT_ERR_UNSUPPORTED, "adaptive sampling in the f32 mode");
    // a pass: the tail of the frame's tile order as one tile shard
    rt_render_params rp = *p;
    rp.row_stride = 1;
    rp.row_block = 0;
    rp.tile_shard = 1;
    rp.count_work = 0;

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;

    AdaptiveBlock fr;   // (of the call's own: freed on every way out)
    HIP_TRY(fr.init(p->width, p->height, hv != nullptr, &stream));
    AdaptiveAdvance adv;
    rc = fr.advance(c, cam, rp, sched, ap->threshold, p->spp, 0, nullptr, false, stream, adv);
    if (rc) return rc;
    rc = fr.resolve(p->out_format, p->out_on_device != 0, out, hv, c->out_buf, stream);
    if (rc) return rc;
    rc = scope.end();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(stream));

    adaptive_last_stats(c, adv, p->spp, sched.chunk, fr.n_tiles);
    rt_adaptive_stats as{};
    as.min_spp = sched.min_r;
    as.step_spp = sched.step_r;
    as.spp_chunk = sched.chunk;
    as.tiles = fr.n_tiles;
    as.samples_uniform = (uint64_t)p->width * (uint64_t)p->height * (uint64_t)p->spp;
    as.passes = adv.launches;
    as.max_pass_batches = adv.max_launch_batches;
    as.samples_traced = adv.samples;
    as.trace_ms = adv.trace_ms;
    as.moments_ms = adv.moments_ms;
    as.classify_ms = adv.classify_ms;
    c->astats = as;
    return RT_OK;
}

extern "C" {

int rt_render_adaptive(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_adaptive_params* ap,
                       const rt_adaptive_out* out)
{
    return render_adaptive(c, cam, p, ap, out, nullptr);
}

int rt_render_adaptive_halves(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_adaptive_params* ap,
                              const rt_adaptive_out* out, const rt_adaptive_halves* halves)
{
    if (!halves || !halves->mean_a || !halves->mean_b) return fail(RT_ERR_INVALID, "null argument");
    if (halves->mean_a == halves->mean_b || (out && (halves->mean_a == out->mean || halves->mean_b == out->mean)))
        return fail(RT_ERR_INVALID, "rt_adaptive_halves: mean_a, mean_b and the mean must be three buffers");
    return render_adaptive(c, cam, p, ap, out, halves);
}

int rt_adaptive_last_stats(rt_ctx* c, rt_adaptive_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    *out = c->astats;
    return RT_OK;
}

// ---- first-hit feature buffers (rt_abi.h; features_device.hpp, features_kernel.hip) -------------
// The launch is the chunk schedule's, planned as one (rtp::plan with the schedule set to CHUNKS:
// the kernel variant, the slab precision, what is staged in LDS), on the context's trace-output
// buffer: 7 doubles per (pixel, chunk), in batches on chunk boundaries when they exceed the
// buffer's bound, the running sums then carried in acc_tmp. Events: ev_ft[0] before the first
// trace_features launch, ev_ft[1] after the last one, ev_ft[2] after the last reduction.
int rt_render_features(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_features_out* out)
{
    if (!c || !cam || !p || !out) return fail(RT_ERR_INVALID, "null argument");
    if (!out->albedo && !out->normal && !out->depth) return fail(RT_ERR_INVALID, "rt_features_out: every output is null");
    if (!c->has_scene) return fail(RT_ERR_NO_SCENE, "no scene uploaded");
    if (p->row_begin != 0 || (p->row_stride != 0 && p->row_stride != 1) || p->row_block < 0 || p->row_block > 1 ||
        p->tile_shard != 0)
        return fail(RT_ERR_INVALID, "rt_render_features renders whole frames: the shard fields must be unset");
    rt_render_params rp = *p;
    rp.row_stride = 1;
    rp.row_block = 0;
    rp.count_work = 0;
    if (bad_geometry(&rp) || p->spp < 1) return fail(RT_ERR_INVALID, "bad render params (rt_render_features needs spp >= 1)");
    if (c->opt.precision == RT_PREC_F32) return fail(RT_ERR_UNSUPPORTED, "feature buffers in the f32 mode");
    const Layout lay = layout_of(&rp);
    const int W = p->width, H = p->height;
    if (lay.w != W || lay.rows != H) return fail(RT_ERR_INVALID, "bad render params");
    const long long n_px = (long long)W * H;
    const int chunk = p->spp_chunk > 0 ? std::min(p->spp_chunk, p->spp) : auto_chunk(p->spp);
    const int n_chunks = (p->spp + chunk - 1) / chunk;
    const bool on_dev = p->out_on_device != 0;

    rtp::Options opt = c->opt;
    opt.schedule = RT_SCHED_CHUNKS;
    rtp::Request rq;
    rq.lay = lay;
    rq.s_begin = 0;
    rq.s_end = p->spp;
    rq.chunk = chunk;
    rq.cam_mag = rtp::camera_magnitude(*cam);
    rq.cam_time0 = cam->time0;
    rq.cam_time1 = cam->time1;
    const rtp::Plan pl = rtp::plan(c->scene, c->dev, opt, rq, rtp::Retry{c->sample_buf_cap, false});
    if (pl.err) return fail(pl.err, pl.err_msg);

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;

    // chunks per batch: what the trace-output bound holds (at least one)
    const size_t chunk_bytes = (size_t)n_px * rtk::kFeatureChannels * sizeof(double);
    const int batch = (int)std::min<size_t>((size_t)n_chunks, std::max<size_t>(1, c->sample_buf_cap / chunk_bytes));
    const int n_batches = (n_chunks + batch - 1) / batch;
    rc = c->partial.reserve(stream, (size_t)batch * chunk_bytes);
    if (rc) return rc;
    if (n_batches > 1) {
        rc = c->acc_tmp.reserve(stream, chunk_bytes);
        if (rc) return rc;
    }
    // host-bound frames: staged [albedo | normal | depth] in the context's output buffer
    const size_t px = (size_t)n_px;
    double *d_albedo = out->albedo, *d_normal = out->normal, *d_depth = out->depth;
    if (!on_dev) {
        rc = c->out_buf.reserve(stream, std::max<size_t>(7 * px * sizeof(double), 16));
        if (rc) return rc;
        double* s = c->out_buf.as<double>();
        d_albedo = out->albedo ? s : nullptr;
        d_normal = out->normal ? s + 3 * px : nullptr;
        d_depth = out->depth ? s + 6 * px : nullptr;
    }

    const int64_t img_tiles = (int64_t)((W + 7) / 8) * ((H + 7) / 8);
    rtk::KParams K;
    rc = fill_kparams(c, cam, &rp, lay, chunk, Sink{}, img_tiles, K);
    if (rc) return rc;
    // (the plan of the chunk schedule in f64: no staged sample starts, nothing counted)
    const PlannedLaunch launch = planned_launch(c->S, pl);
    const rtk::SceneDev& S = launch.S;
    const rtk::LaunchOpts& o = launch.o;

    HIP_TRY(c->ev_ft.record(0, stream));
    for (int bi = 0; bi < n_batches; ++bi) {
        const int c0 = bi * batch, c1 = std::min(n_chunks, c0 + batch);
        K.sample_begin = c0 * chunk;
        K.spp = (int)std::min<long long>(p->spp, (long long)c1 * chunk);
        K.n_chunks = c1 - c0;
        rtk::KParams* dK = c->params.as<rtk::KParams>() + c->param_slot;
        c->param_slot = (c->param_slot + 1) % kParamSlots;
        HIP_TRY(hipMemcpyAsync(dK, &K, sizeof K, hipMemcpyHostToDevice, stream));
        HIP_TRY(rtk::launch_features(S, K, dK, c->partial.as<double>(), o, stream));
        if (bi == n_batches - 1) HIP_TRY(c->ev_ft.record(1, stream));
        HIP_TRY(rtk::launch_reduce_features(c->partial.as<double>(), c->acc_tmp.as<double>(), d_albedo, d_normal, d_depth,
                                            n_px, K.n_chunks, bi == 0, bi == n_batches - 1, 1.0 / (double)p->spp, stream));
    }
    HIP_TRY(c->ev_ft.record(2, stream));
    c->fstats = rt_features_stats{};
    c->fstats.samples = (uint64_t)n_px * (uint64_t)p->spp;
    c->fstats.variant_features = (int32_t)pl.variant;
    c->fstats.spp_chunk = chunk;
    c->ev_ft.arm();
    if (!on_dev) {
        if (out->albedo) HIP_TRY(hipMemcpyAsync(out->albedo, d_albedo, 3 * px * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (out->normal) HIP_TRY(hipMemcpyAsync(out->normal, d_normal, 3 * px * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (out->depth) HIP_TRY(hipMemcpyAsync(out->depth, d_depth, px * sizeof(double), hipMemcpyDeviceToHost, stream));
    }
    rc = scope.end();
    if (rc) return rc;
    if (!on_dev) HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

int rt_features_last_stats(rt_ctx* c, rt_features_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    if (c->ev_ft.pending) {
        HIP_TRY(hipSetDevice(c->device));
        float ms[2] = {0, 0};
        const int rc = c->ev_ft.resolve(ms);
        if (rc) return rc;
        c->fstats.kernel_ms = ms[0];
        c->fstats.reduce_ms = ms[1];
    }
    *out = c->fstats;
    return RT_OK;
}

}  // extern "C"

// ---- ray queries (rt_abi.h; query_device.hpp, query_kernel.hip) ---------------------------------
// The host's statement of "Invalid rays" (rt_abi.h) but for the origin bound: what a host-pointer
// call plans from (the largest |o component| and the |d| range of the rays that will be walked) and
// the invalid count of a call that brings no records back.
namespace {

struct RayScan {
    int64_t invalid = 0;
    double o_max = 0.0;                  // the largest |o component| of the valid rays
    bool d_in_f32_range = true;          // every valid ray's largest |d component| is within [2^-40, 2^40]
};

RayScan scan_rays(const rt_ray* rays, int64_t n, const rtp::SceneFacts& scene)
{
    RayScan s;
    for (int64_t i = 0; i < n; ++i) {
        const rt_ray& r = rays[i];
        bool ok = std::isfinite(r.time);
        for (int a = 0; a < 3; ++a) ok = ok && std::isfinite(r.o[a]) && std::isfinite(r.d[a]);
        const double dm = std::fmax(std::fmax(std::fabs(r.d[0]), std::fabs(r.d[1])), std::fabs(r.d[2]));
        ok = ok && dm > 0.0 && r.t_min <= r.t_max;
        if (scene.has_moving) ok = ok && r.time >= scene.time_lo && r.time <= scene.time_hi;
        if (!ok) {
            s.invalid++;
            continue;
        }
        s.o_max = std::fmax(s.o_max, std::fmax(std::fmax(std::fabs(r.o[0]), std::fabs(r.o[1])), std::fabs(r.o[2])));
        s.d_in_f32_range = s.d_in_f32_range && dm >= 0x1.0p-40 && dm <= 0x1.0p+40;
    }
    return s;
}

}  // namespace

extern "C" {

// The launch is planned as a chunk-schedule launch is (rtp::plan: the kernel variant, the slab
// precision, what is staged in LDS), with the rays' origin bound in the camera's place. Device
// pointers: one launch on the caller's arrays, timed by ev_q. Host pointers: batches of rays whose
// device copies — the rays, then each output — fit RT_OPT_TRACE_BUF_BYTES, in the context's query
// buffer; each batch is copied in, traced between ev_q's two events and copied back, and the
// batches' kernel times add up.
int rt_trace_rays(rt_ctx* c, const rt_query_params* p, const rt_ray* rays, const rt_query_out* out)
{
    if (!c || !p || !rays || !out) return fail(RT_ERR_INVALID, "null argument");
    if (p->mode != RT_QUERY_CLOSEST && p->mode != RT_QUERY_ANY) return fail(RT_ERR_INVALID, "rt_query_params.mode");
    const bool any = p->mode == RT_QUERY_ANY;
    if (!any && ((!out->hits && !out->albedo) || out->occluded))
        return fail(RT_ERR_INVALID, "RT_QUERY_CLOSEST writes hits or albedo (at least one) and no occluded bytes");
    if (any && (!out->occluded || out->hits || out->albedo))
        return fail(RT_ERR_INVALID, "RT_QUERY_ANY writes occluded bytes only");
    if (p->n < 0 || p->n > 0x7fffffffLL) return fail(RT_ERR_INVALID, "rt_query_params.n: 0 .. 2^31 - 1 rays");
    const bool on_dev = p->on_device != 0;
    if (on_dev && (((uintptr_t)rays & 15) || ((uintptr_t)out->hits & 15)))
        return fail(RT_ERR_INVALID, "device ray and hit records must be 16-byte aligned");
    if (!c->has_scene) return fail(RT_ERR_NO_SCENE, "no scene uploaded");
    if (c->opt.precision == RT_PREC_F32) return fail(RT_ERR_UNSUPPORTED, "ray queries in the f32 mode");
    const int64_t n = p->n;
    c->ev_q.disarm();
    c->qstats = rt_query_stats{};
    c->qstats.mode = p->mode;
    c->qstats.invalid = on_dev ? -1 : 0;
    if (n == 0) return RT_OK;

    // the origin bound the launch is planned with, and whether every |d| suits f32 slabs
    RayScan scan;
    double bound = p->origin_bound;
    const bool bound_known = on_dev ? std::isfinite(bound) && bound > 0.0 : true;
    if (!on_dev) {
        scan = scan_rays(rays, n, c->scene);
        bound = scan.o_max;
    }
    rtp::Options opt = c->opt;
    opt.schedule = RT_SCHED_CHUNKS;
    if (!bound_known || !scan.d_in_f32_range) opt.slab32 = 0;
    rtp::Request rq;
    rq.lay = Layout{8, 8};
    rq.s_begin = 0;
    rq.s_end = 1;
    rq.chunk = 1;
    rq.cam_mag = bound_known ? bound : 0.0;
    rq.cam_time0 = c->scene.time_lo;   // (ray times are checked per ray, in the kernel)
    rq.cam_time1 = c->scene.time_hi;
    // The query's walk tests every instance where it meets it, its BLAS walk nested at blas_base;
    // the scene's stack_entries may be the trace kernels' smaller count, which relies on their
    // deferred first instance. So the launch is planned (LDS or scratch stack, the LDS left for
    // BLAS nodes) and laid out with the entries of the nested walk.
    rtp::SceneFacts facts = c->scene;
    facts.stack_entries = facts.nested_stack_entries;
    const rtp::Plan pl = rtp::plan(facts, c->dev, opt, rq, rtp::Retry{c->sample_buf_cap, false});
    if (pl.err) return fail(pl.err, pl.err_msg);
    PlannedLaunch launch = planned_launch(c->S, pl);
    launch.S.stack_entries = facts.stack_entries;

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;

    rtk::QueryArgs Q{};
    Q.seed = p->seed;
    Q.bounce = p->bounce;
    Q.has_moving = c->scene.has_moving;
    Q.time_lo = c->scene.time_lo;
    Q.time_hi = c->scene.time_hi;
    Q.origin_bound = bound_known ? bound : (double)INFINITY;
    c->qstats.rays = n;
    c->qstats.variant_features = (int32_t)pl.variant;
    c->qstats.slab32 = pl.slab32;

    if (on_dev) {
        Q.rays = rays;
        Q.hits = out->hits;
        Q.albedo = out->albedo;
        Q.occluded = out->occluded;
        Q.n = n;
        HIP_TRY(c->ev_q.record(0, stream));
        HIP_TRY(rtk::launch_query(launch.S, Q, p->mode, launch.o, stream));
        HIP_TRY(c->ev_q.record(1, stream));
        c->ev_q.arm();
        c->qstats.batches = 1;
        return scope.end();
    }

    // a batch's device copies: [rays][hits][albedo][occluded], each on a 256-byte boundary
    const size_t per_ray = sizeof(rt_ray) + (out->hits ? sizeof(rt_hit) : 0) + (out->albedo ? 3 * sizeof(double) : 0) + (any ? 1 : 0);
    const int64_t batch = (int64_t)std::min<size_t>((size_t)n, std::max<size_t>(1, c->sample_buf_cap / per_ray));
    const size_t off_hits = align_up((size_t)batch * sizeof(rt_ray), 256);
    const size_t off_albedo = off_hits + (out->hits ? align_up((size_t)batch * sizeof(rt_hit), 256) : 0);
    const size_t off_occ = off_albedo + (out->albedo ? align_up((size_t)batch * 3 * sizeof(double), 256) : 0);
    rc = c->query_buf.reserve(stream, off_occ + (any ? align_up((size_t)batch, 256) : 0));
    if (rc) return rc;
    char* const base = c->query_buf.as<char>();
    Q.rays = reinterpret_cast<const rt_ray*>(base);
    Q.hits = out->hits ? reinterpret_cast<rt_hit*>(base + off_hits) : nullptr;
    Q.albedo = out->albedo ? reinterpret_cast<double*>(base + off_albedo) : nullptr;
    Q.occluded = any ? reinterpret_cast<uint8_t*>(base + off_occ) : nullptr;
    double kernel_ms = 0.0;
    for (int64_t b0 = 0; b0 < n; b0 += batch) {
        const size_t m = (size_t)std::min<int64_t>(batch, n - b0);
        Q.n = (long long)m;
        HIP_TRY(hipMemcpyAsync(base, rays + b0, m * sizeof(rt_ray), hipMemcpyHostToDevice, stream));
        HIP_TRY(c->ev_q.record(0, stream));
        HIP_TRY(rtk::launch_query(launch.S, Q, p->mode, launch.o, stream));
        HIP_TRY(c->ev_q.record(1, stream));
        if (out->hits) HIP_TRY(hipMemcpyAsync(out->hits + b0, Q.hits, m * sizeof(rt_hit), hipMemcpyDeviceToHost, stream));
        if (out->albedo) HIP_TRY(hipMemcpyAsync(out->albedo + 3 * b0, Q.albedo, m * 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
        if (any) HIP_TRY(hipMemcpyAsync(out->occluded + b0, Q.occluded, m, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));   // the next batch reuses the buffer
        float ms = 0.0f;
        HIP_TRY(c->ev_q.elapsed(0, &ms));
        kernel_ms += ms;
        c->qstats.batches++;
    }
    rc = scope.end();
    if (rc) return rc;
    c->qstats.kernel_ms = kernel_ms;
    c->qstats.invalid = scan.invalid;
    if (out->hits) {   // counted from the flags that came back
        c->qstats.invalid = 0;
        for (int64_t i = 0; i < n; ++i) c->qstats.invalid += (out->hits[i].flags & RT_HIT_INVALID) != 0;
    }
    return RT_OK;
}

int rt_query_last_stats(rt_ctx* c, rt_query_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    if (c->ev_q.pending) {
        HIP_TRY(hipSetDevice(c->device));
        float ms[1] = {0};
        const int rc = c->ev_q.resolve(ms);
        if (rc) return rc;
        c->qstats.kernel_ms = ms[0];
    }
    *out = c->qstats;
    return RT_OK;
}

}  // extern "C"
