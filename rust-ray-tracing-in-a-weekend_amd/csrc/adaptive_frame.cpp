// adaptive_frame.cpp — see adaptive_frame.hpp
#include "adaptive_frame.hpp"

#include <algorithm>
#include <vector>

#include "render_internal.hpp"

hipError_t AdaptiveBlock::init(int width_, int height_, bool with_halves_, const hipStream_t* on_stream)
{
    const AdaptiveLayout L(width_, height_, with_halves_);
    width = width_;
    height = height_;
    n_tiles = (int)L.nt;
    with_halves = with_halves_;
    std::vector<uint32_t> raster(L.nt);
    for (size_t i = 0; i < L.nt; ++i) raster[i] = (uint32_t)i;
    hipError_t e = blk.alloc(L.bytes());
    if (e != hipSuccess) return e;
    double* d = blk.as<double>();
    uint32_t* u = (uint32_t*)(d + L.n_f64);
    if (on_stream) {
        e = hipMemsetAsync(blk.p, 0, L.bytes(), *on_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(u + L.order, raster.data(), L.nt * sizeof(uint32_t), hipMemcpyHostToDevice, *on_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(*on_stream);   // (raster is read until the copy is done)
    } else {
        e = hipMemset(blk.p, 0, L.bytes());
        if (e == hipSuccess) e = hipMemcpy(u + L.order, raster.data(), L.nt * sizeof(uint32_t), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = ev.create();
    if (e != hipSuccess) return e;
    F.sum = d + L.sum;
    F.sum_open = d + L.sum_open;
    F.q = d + L.q;
    F.q_open = d + L.q_open;
    F.tile_error = d + L.tile_error;
    error_in = d + L.error_in;
    if (with_halves) {
        Hf.sum_a = d + L.sum_a;
        Hf.sum_a_open = d + L.sum_a_open;
        Hf.sum_b = d + L.sum_b;
        Hf.sum_b_open = d + L.sum_b_open;
    }
    F.tile_spp = u + L.tile_spp;
    order = u + L.order;
    mask = u + L.mask;
    record = (rtk::RegroupRecord*)(u + L.record);
    F.order = order;
    F.width = width;
    F.height = height;
    F.tiles_x = (width + 7) / 8;
    return hipSuccess;
}

int AdaptiveBlock::advance(rt_ctx* c, const rt_camera* cam, const rt_render_params& rp_in, const rtas::Schedule& s,
                           double threshold, int cap, int max_launches, const double* map, bool map_on_device,
                           hipStream_t stream, AdaptiveAdvance& a)
{
    a = AdaptiveAdvance{};
    a.active_left = n_tiles;
    uint32_t* const by_mask = map ? mask : nullptr;
    if (map) {   // the selected set, fixed here
        if (!map_on_device) {
            HIP_TRY(hipMemcpyAsync(error_in, map, (size_t)n_tiles * sizeof(double), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));   // (the caller's array is read until the copy is done)
            map = error_in;
        }
        HIP_TRY(rtk::launch_adaptive_select_mask(F.tile_spp, map, mask, n_tiles, threshold, (uint32_t)cap, stream));
    }

    // a regroup and its record: one synchronization
    rtk::RegroupRecord rec{};
    auto regroup = [&]() -> int {
        HIP_TRY(ev.record(0, stream));
        HIP_TRY(rtk::launch_adaptive_regroup(F.tile_spp, F.tile_error, by_mask, order, n_tiles, threshold, (uint32_t)cap,
                                             record, stream));
        HIP_TRY(hipMemcpyAsync(&rec, record, sizeof rec, hipMemcpyDeviceToHost, stream));
        HIP_TRY(ev.record(1, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float t_classify = 0;
        HIP_TRY(ev.elapsed(0, &t_classify));
        a.classify_ms += t_classify;
        order_is_raster = false;
        if (rec.n_group > (uint32_t)n_tiles || rec.n_active > (uint32_t)n_tiles || rec.n_group > rec.n_active ||
            (rec.n_group > 0 && rec.n_star >= (uint32_t)cap))
            return fail(RT_ERR_HIP, "adaptive regroup: inconsistent record");
        min_count = rec.n_min;
        max_count = rec.n_max;
        a.active_left = (int32_t)rec.n_active;
        return RT_OK;
    };
    if (!map && max_count == 0 && order_is_raster) {
        // a fresh frame: every tile at 0, the group is the frame in the raster order init wrote
        rec.n_group = rec.n_active = (uint32_t)n_tiles;
    } else {
        const int rc = regroup();
        if (rc) return rc;
    }

    rt_render_params rp = rp_in;   // a launch: the tail of the tile order as one tile shard
    rp.stream = stream;
    while (rec.n_group > 0 && (max_launches == 0 || a.launches < max_launches)) {
        const int first = (int)rec.n_star, end = rtas::next_count(first, cap, s.min_r, s.step_r);
        const int n_group = (int)rec.n_group;
        rp.row_begin = n_tiles - n_group;
        rp.spp = end;
        F.pos_begin = n_tiles - n_group;
        Sink sink;
        sink.moments = &F;
        sink.n_done = end;
        sink.halves = with_halves ? &Hf : nullptr;
        int rc = run_range(c, cam, &rp, first, end, s.chunk, stream, sink);
        if (rc) return rc;
        ragged_cap = rtas::ragged_after(ragged_cap, end, s.chunk);
        const int trace_batches = c->stats.n_batches;
        rc = regroup();
        if (rc) return rc;
        float t_trace = 0, t_moments = 0;
        HIP_TRY(c->ev.elapsed(0, &t_trace));   // (the launch's render span, read here: disarmed by adaptive_last_stats)
        HIP_TRY(c->ev.elapsed(1, &t_moments));
        a.trace_ms += t_trace;
        a.moments_ms += t_moments;
        a.launches += 1;
        a.samples += 64ull * (uint64_t)n_group * (uint64_t)(end - first);
        a.batches += trace_batches;
        a.max_launch_batches = std::max(a.max_launch_batches, trace_batches);
    }
    return RT_OK;
}

int AdaptiveBlock::resolve(int out_format, bool on_dev, const rt_adaptive_out* out, const rt_adaptive_halves* hv,
                           DevBuf& stage, hipStream_t stream)
{
    const bool f64 = out_format == RT_OUT_F64;
    const size_t hw = (size_t)width * (size_t)height, nt = (size_t)n_tiles;
    const size_t mean_bytes = hw * 3 * (f64 ? 8 : 4);
    // host-bound outputs: staged [mean | halves: mean_a | mean_b | se], a frame of f64 each at the most
    void *dev_mean = out->mean, *dev_a = hv ? hv->mean_a : nullptr, *dev_b = hv ? hv->mean_b : nullptr;
    double* dev_se = out->stderr_map;
    if (!on_dev) {
        const size_t n_means = hv ? 9 * hw : 3 * hw;
        const int rc = stage.reserve(stream, (n_means + (out->stderr_map ? hw : 0)) * sizeof(double));
        if (rc) return rc;
        double* st = stage.as<double>();
        dev_mean = st;
        dev_a = st + 3 * hw;
        dev_b = st + 6 * hw;
        dev_se = out->stderr_map ? st + n_means : nullptr;
    }
    HIP_TRY(rtk::launch_adaptive_resolve(F.sum, F.q, F.tile_spp, dev_mean, f64, dev_se, width, height, stream));
    const hipMemcpyKind kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!on_dev) {
        HIP_TRY(hipMemcpyAsync(out->mean, dev_mean, mean_bytes, kind, stream));
        if (out->stderr_map) HIP_TRY(hipMemcpyAsync(out->stderr_map, dev_se, hw * sizeof(double), kind, stream));
    }
    if (out->tile_spp) HIP_TRY(hipMemcpyAsync(out->tile_spp, F.tile_spp, nt * sizeof(uint32_t), kind, stream));
    if (out->tile_error) HIP_TRY(hipMemcpyAsync(out->tile_error, F.tile_error, nt * sizeof(double), kind, stream));
    if (hv) {
        HIP_TRY(rtk::launch_adaptive_resolve_halves(Hf.sum_a, Hf.sum_b, F.tile_spp, dev_a, dev_b, f64, width, height, stream));
        if (!on_dev) {
            HIP_TRY(hipMemcpyAsync(hv->mean_a, dev_a, mean_bytes, kind, stream));
            HIP_TRY(hipMemcpyAsync(hv->mean_b, dev_b, mean_bytes, kind, stream));
        }
    }
    return RT_OK;
}

void adaptive_last_stats(rt_ctx* c, const AdaptiveAdvance& a, int cap, int chunk, int n_tiles)
{
    c->stats.kernel_ms = a.trace_ms;
    c->stats.reduce_ms = a.moments_ms;
    c->stats.samples = a.samples;
    c->stats.n_batches = a.batches;
    c->stats.n_chunks = (cap + chunk - 1) / chunk;
    c->stats.n_items = 64ull * (uint64_t)n_tiles * (uint64_t)c->stats.n_chunks;
    c->stats.casts = c->stats.node_visits = c->stats.prim_tests = 0;
    c->ev.disarm();
    c->pending_counts = false;
}
