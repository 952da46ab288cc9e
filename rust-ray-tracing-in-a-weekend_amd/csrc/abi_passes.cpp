// abi_passes.cpp — the auxiliary passes behind the C ABI (include/rt/rt_abi.h) that render through
// the driver (render_internal.hpp): tile-adaptive sampling and the first-hit feature buffers, with
// their stats.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "rt/rt_abi.h"
#include "adaptive_criterion.hpp"
#include "ctx_internal.hpp"
#include "features_kernel.hpp"
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

// rt_render_adaptive (hv null) and rt_render_adaptive_halves: one driver, the second with the two
// half sums carried beside the frame's moments and resolved after them
static int render_adaptive(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_adaptive_params* ap,
                           const rt_adaptive_out* out, const rt_adaptive_halves* hv)
{
    if (!c || !cam || !p || !ap || !out || !out->mean) return fail(RT_ERR_INVALID, "null argument");
    if (!c->has_scene) return fail(RT_ERR_NO_SCENE, "no scene uploaded");
    if (p->row_begin != 0 || (p->row_stride != 0 && p->row_stride != 1) || p->row_block < 0 || p->row_block > 1 ||
        p->tile_shard != 0)
        return fail(RT_ERR_INVALID, "rt_render_adaptive renders whole frames: the shard fields must be unset");
    // a pass: the tail of the call's tile order as one tile shard
    rt_render_params rp = *p;
    rp.row_stride = 1;
    rp.row_block = 0;
    rp.tile_shard = 1;
    rp.count_work = 0;
    if (bad_geometry(&rp) || p->spp < 2 || p->max_depth < 0 || (p->out_format != RT_OUT_F32 && p->out_format != RT_OUT_F64))
        return fail(RT_ERR_INVALID, "bad render params (adaptive sampling needs spp >= 2)");
    if (ap->min_spp < 2 || ap->step_spp < 1 || std::isnan(ap->threshold))
        return fail(RT_ERR_INVALID, "bad adaptive params (min_spp >= 2, step_spp >= 1, threshold not NaN)");
    if (c->opt.precision == RT_PREC_F32) return fail(RT_ERR_UNSUPPORTED, "adaptive sampling in the f32 mode");
    const int W = p->width, H = p->height, tiles_x = (W + 7) / 8;
    const long long tiles_ll = (long long)tiles_x * ((H + 7) / 8);
    if (tiles_ll > 0x3fffffffLL) return fail(RT_ERR_INVALID, "too many tiles");
    const int n_tiles = (int)tiles_ll;
    const int chunk = p->spp_chunk > 0 ? std::min(p->spp_chunk, p->spp) : auto_chunk(p->spp);
    auto rounded = [&](int v) { return (int)std::min<long long>(p->spp, ((long long)v + chunk - 1) / chunk * chunk); };
    const int min_r = rounded(ap->min_spp), step_r = rounded(ap->step_spp);
    const bool on_dev = p->out_on_device != 0;

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;

    // device state: [sum | sum_open | q | q_open | tile_error | se map (host-bound only) | halves:
    // sum_a | sum_a_open | sum_b | sum_b_open | the two half means (host-bound only)] f64, then
    // [tile_spp | order A | order B | counts] u32; zeroed: the sums start from 0.0
    const size_t hw = (size_t)W * (size_t)H, nt = (size_t)n_tiles;
    const bool own_se = out->stderr_map && !on_dev;
    const size_t n_base = 8 * hw + nt + (own_se ? hw : 0);
    const size_t n_f64 = n_base + (hv ? 12 * hw + (on_dev ? 0 : 6 * hw) : 0), n_u32 = 3 * nt + 2;
    DevBuf blk;   // (of the call's own: freed on every way out)
    HIP_TRY(blk.alloc(n_f64 * sizeof(double) + n_u32 * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(blk.p, 0, n_f64 * sizeof(double) + n_u32 * sizeof(uint32_t), stream));
    double* d = (double*)blk.p;
    rtk::AdaptiveFrame F{};
    F.sum = d;
    F.sum_open = d + 3 * hw;
    F.q = d + 6 * hw;
    F.q_open = d + 7 * hw;
    F.tile_error = d + 8 * hw;
    double* se_dev = out->stderr_map ? (on_dev ? out->stderr_map : d + 8 * hw + nt) : nullptr;
    uint32_t* u = (uint32_t*)(d + n_f64);
    F.tile_spp = u;
    uint32_t* order[2] = {u + nt, u + 2 * nt};
    uint32_t* counts = u + 3 * nt;
    F.width = W;
    F.height = H;
    F.tiles_x = tiles_x;
    rtk::AdaptiveHalves Hf{};
    if (hv) {
        Hf.sum_a = d + n_base;
        Hf.sum_a_open = d + n_base + 3 * hw;
        Hf.sum_b = d + n_base + 6 * hw;
        Hf.sum_b_open = d + n_base + 9 * hw;
    }
    {
        std::vector<uint32_t> raster(nt);
        for (size_t i = 0; i < nt; ++i) raster[i] = (uint32_t)i;
        HIP_TRY(hipMemcpyAsync(order[0], raster.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));   // (raster is read until the copy is done)
    }
    EventSpan<2> ev;   // around a pass's classification
    HIP_TRY(ev.create());

    rt_adaptive_stats as{};
    as.min_spp = min_r;
    as.step_spp = step_r;
    as.spp_chunk = chunk;
    as.tiles = n_tiles;
    as.samples_uniform = (uint64_t)hw * (uint64_t)p->spp;
    int done = 0, n_stopped = 0, cur = 0, batches = 0;
    while (n_stopped < n_tiles && done < p->spp) {
        const int end = std::min(p->spp, done + (done == 0 ? min_r : step_r));
        rp.row_begin = n_stopped;
        F.order = order[cur];
        F.pos_begin = n_stopped;
        Sink sink;
        sink.moments = &F;
        sink.n_done = end;
        sink.halves = hv ? &Hf : nullptr;
        rc = run_range(c, cam, &rp, done, end, chunk, stream, sink);
        if (rc) return rc;
        HIP_TRY(ev.record(0, stream));
        HIP_TRY(rtk::launch_adaptive_compact(order[cur], order[cur ^ 1], F.tile_error, n_tiles, n_stopped, ap->threshold,
                                             end >= p->spp, counts, stream));
        uint32_t h_counts[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(h_counts, counts, sizeof h_counts, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ev.record(1, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float t_trace = 0, t_moments = 0, t_classify = 0;
        HIP_TRY(c->ev.elapsed(0, &t_trace));   // (the pass's render span, read here: disarmed below)
        HIP_TRY(c->ev.elapsed(1, &t_moments));
        HIP_TRY(ev.elapsed(0, &t_classify));
        as.trace_ms += t_trace;
        as.moments_ms += t_moments;
        as.classify_ms += t_classify;
        as.passes += 1;
        as.max_pass_batches = std::max(as.max_pass_batches, c->stats.n_batches);
        as.samples_traced += 64ull * (uint64_t)(n_tiles - n_stopped) * (uint64_t)(end - done);
        batches += c->stats.n_batches;
        if ((int)h_counts[0] < n_stopped || h_counts[0] + h_counts[1] != (uint32_t)n_tiles)
            return fail(RT_ERR_HIP, "adaptive compact: inconsistent tile counts");
        n_stopped = (int)h_counts[0];
        cur ^= 1;
        done = end;
    }

    const size_t mean_bytes = hw * 3 * (p->out_format == RT_OUT_F64 ? 8 : 4);
    void* dev_mean = out->mean;
    if (!on_dev) {
        rc = c->out_buf.reserve(stream, std::max<size_t>(mean_bytes, 16));
        if (rc) return rc;
        dev_mean = c->out_buf.p;
    }
    HIP_TRY(rtk::launch_adaptive_resolve(F.sum, F.q, F.tile_spp, dev_mean, p->out_format == RT_OUT_F64, se_dev, W, H, stream));
    const hipMemcpyKind kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!on_dev) HIP_TRY(hipMemcpyAsync(out->mean, dev_mean, mean_bytes, kind, stream));
    if (own_se) HIP_TRY(hipMemcpyAsync(out->stderr_map, se_dev, hw * sizeof(double), kind, stream));
    if (out->tile_spp) HIP_TRY(hipMemcpyAsync(out->tile_spp, F.tile_spp, nt * sizeof(uint32_t), kind, stream));
    if (out->tile_error) HIP_TRY(hipMemcpyAsync(out->tile_error, F.tile_error, nt * sizeof(double), kind, stream));
    if (hv) {
        void* dev_a = on_dev ? hv->mean_a : (void*)(d + n_base + 12 * hw);
        void* dev_b = on_dev ? hv->mean_b : (void*)(d + n_base + 15 * hw);
        HIP_TRY(rtk::launch_adaptive_resolve_halves(Hf.sum_a, Hf.sum_b, F.tile_spp, dev_a, dev_b,
                                                    p->out_format == RT_OUT_F64, W, H, stream));
        if (!on_dev) {
            HIP_TRY(hipMemcpyAsync(hv->mean_a, dev_a, mean_bytes, kind, stream));
            HIP_TRY(hipMemcpyAsync(hv->mean_b, dev_b, mean_bytes, kind, stream));
        }
    }
    rc = scope.end();
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(stream));

    // rt_last_stats: the call as a whole (the variant fields are the last pass's)
    c->stats.kernel_ms = as.trace_ms;
    c->stats.reduce_ms = as.moments_ms;
    c->stats.samples = as.samples_traced;
    c->stats.n_batches = batches;
    c->stats.n_chunks = (p->spp + chunk - 1) / chunk;
    c->stats.n_items = 64ull * (uint64_t)n_tiles * (uint64_t)c->stats.n_chunks;
    c->stats.casts = c->stats.node_visits = c->stats.prim_tests = 0;
    c->ev.disarm();
    c->pending_counts = false;
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
