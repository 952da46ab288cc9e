// abi_filters.cpp — the post-filters behind the C ABI (include/rt/rt_abi.h): the variance-guided
// NL-means filter (rt_denoise, rt_denoise_guided; denoise_kernel.hip), the variance-guided
// a-trous wavelet filter (rt_denoise_atrous; atrous_kernel.hip), the cross-filtered NL-means over
// two half frames (rt_denoise_cross; cross_kernel.hip) and the multi-scale NL-means
// (rt_denoise_pyramid; pyramid_kernel.hip), with their stats: each entry is its own check, scratch
// size, launch and stats fields around one call frame (FilterCall). Their host counterparts are
// denoise_host.cpp, atrous_host.cpp, cross_host.cpp and pyramid_host.cpp.
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "rt/rt_abi.h"
#include "atrous.hpp"
#include "cross.hpp"
#include "ctx_internal.hpp"
#include "denoise.hpp"
#include "filter_guides.hpp"
#include "pyramid.hpp"

namespace {

// rt_denoise_host and rt_denoise_atrous_host live in files that link without this one: their error
// text comes through a hook
[[maybe_unused]] const bool g_filter_sink_set = (rtk::filter_error_sink = [](const char* msg) { (void)fail(0, msg); }, true);

// A call's host-pointer arguments staged in one device block of the call's own. stage() lays the
// parts given (a null host pointer: no part) out 256-byte aligned, makes the one allocation and
// enqueues the host-to-device copies of the inputs; dev(i) is part i's device address (null for
// no part); copy_back() enqueues the device-to-host copies of the outputs. The block is freed with
// the object, so the object outlives the call's final hipStreamSynchronize.
struct HostStage {
    struct Part {
        const void* host;
        size_t bytes;
        bool out;
        size_t off = 0;
    };
    static constexpr int kMaxParts = 8;
    Part part[kMaxParts];
    int n = 0;
    DevBuf blk;

    int stage(hipStream_t stream, std::initializer_list<Part> parts)
    {
        size_t total = 0;
        for (const Part& q : parts) {
            part[n] = q;
            part[n++].off = total;
            if (q.host) total += align_up(q.bytes, 256);
        }
        HIP_TRY(blk.alloc(total + 256));
        for (int i = 0; i < n; ++i)
            if (part[i].host && !part[i].out)
                HIP_TRY(hipMemcpyAsync(dev(i), part[i].host, part[i].bytes, hipMemcpyHostToDevice, stream));
        return RT_OK;
    }
    void* dev(int i) const { return part[i].host ? blk.as<char>() + part[i].off : nullptr; }
    int copy_back(hipStream_t stream)
    {
        for (int i = 0; i < n; ++i)
            if (part[i].host && part[i].out)
                HIP_TRY(hipMemcpyAsync((void*)part[i].host, dev(i), part[i].bytes, hipMemcpyDeviceToHost, stream));
        return RT_OK;
    }
};

// The frames of a filter call as the kernels take them: the caller's device pointers, or (host
// pointers) their staged copies — the frame, the optional second frame (rt_denoise_cross's other
// half), the map, the result, the optional second result and the guides given.
struct FilterFrames {
    const void *mean, *mean_b;
    const double* se;
    void* out;
    double* se_out;
};

int stage_frames(HostStage& st, hipStream_t stream, size_t hw, size_t frame_bytes, FilterFrames& f, rtk::DenoiseGuides& G)
{
    const size_t b1 = hw * sizeof(double), b3 = 3 * b1;
    const int rc = st.stage(stream, {{f.mean, frame_bytes, false}, {f.mean_b, frame_bytes, false}, {f.se, b1, false},
                                     {f.out, frame_bytes, true}, {f.se_out, b1, true}, {G.albedo, b3, false},
                                     {G.normal, b3, false}, {G.depth, b1, false}});
    if (rc) return rc;
    f = FilterFrames{st.dev(0), st.dev(1), (const double*)st.dev(2), st.dev(3), (double*)st.dev(4)};
    G.albedo = (const double*)st.dev(5);
    G.normal = (const double*)st.dev(6);
    G.depth = (const double*)st.dev(7);
    return RT_OK;
}

// One filter call between its argument check and its return: begin(), the entry's own launch,
// finish(). It owns the call's StreamScope, so the scope ends on every way out once begin() has
// opened it, and its HostStage, so the staged block outlives finish()'s final synchronise. P is
// one of the filters' parameter structs: they share width, height, format, on_device and stream.
struct FilterCall {
    rt_ctx* c;
    hipStream_t stream;
    bool f64, on_dev;
    size_t hw, frame_bytes;
    StreamScope scope;
    HostStage st;
    void* scratch = nullptr;   // the slot's scratch of this call (null for 0 bytes)

    template <typename P>
    FilterCall(rt_ctx* c_, const P& p)
        : c(c_), stream(p.stream ? (hipStream_t)p.stream : c_->stream), f64(p.format == RT_OUT_F64), on_dev(p.on_device != 0),
          hw((size_t)p.width * (size_t)p.height), frame_bytes(hw * 3 * (f64 ? 8 : 4)), scope(c_, stream)
    {
    }

    // In this order: the scope opens; the slot's scratch is grown on demand (its reserve may
    // synchronise the stream, which the scope has ordered after every earlier use); host pointers
    // are staged; the first event is recorded, so the interval is the kernels' alone.
    template <typename Stats>
    int begin(FilterSlot<Stats>& slot, size_t scratch_bytes, FilterFrames& f, rtk::DenoiseGuides& G)
    {
        HIP_TRY(hipSetDevice(c->device));
        int rc = scope.begin();
        if (rc) return rc;
        rc = slot.scratch.reserve(stream, scratch_bytes);
        if (rc) return rc;
        scratch = scratch_bytes ? slot.scratch.p : nullptr;
        if (!on_dev) {
            rc = stage_frames(st, stream, hw, frame_bytes, f, G);
            if (rc) return rc;
        }
        HIP_TRY(slot.ev.record(0, stream));
        return RT_OK;
    }

    // The second event, then the slot's stats become this call's (kernel_ms is read from the armed
    // events later: last_stats), the results are copied back and the scope ends.
    template <typename Stats>
    int finish(FilterSlot<Stats>& slot, const Stats& stats)
    {
        HIP_TRY(slot.ev.record(1, stream));
        slot.stats = stats;
        slot.ev.arm();
        int rc = st.copy_back(stream);
        if (rc) return rc;
        rc = scope.end();
        if (rc) return rc;
        if (!on_dev) HIP_TRY(hipStreamSynchronize(stream));   // (the block is freed once its copies are done)
        return RT_OK;
    }
};

// rt_*_last_stats of a filter: the slot's stats, with kernel_ms read once its events are complete
template <typename Stats>
int last_stats(rt_ctx* c, FilterSlot<Stats> rt_ctx::*slot, Stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    FilterSlot<Stats>& s = c->*slot;
    if (s.ev.pending) {
        HIP_TRY(hipSetDevice(c->device));
        float ms[1] = {0};
        const int rc = s.ev.resolve(ms);
        if (rc) return rc;
        s.stats.kernel_ms = ms[0];
    }
    *out = s.stats;
    return RT_OK;
}

}  // namespace

extern "C" {

// ---- variance-guided NL-means (rt_abi.h: the filter; denoise_kernel.hip; denoise_host.cpp) -------
int rt_denoise_guided(rt_ctx* c, const rt_denoise_params* p, const void* mean, const double* stderr_map,
                      const rt_denoise_guides* g, void* out)
{
    if (!c) return fail(RT_ERR_INVALID, "null argument");
    if (const char* bad = rtk::denoise_check(p, mean, stderr_map, out)) return fail(RT_ERR_INVALID, bad);
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::guides_check(g, G)) return fail(RT_ERR_INVALID, bad);

    FilterCall call(c, *p);
    FilterFrames f{mean, nullptr, stderr_map, out, nullptr};
    const int rc = call.begin(c->flt_denoise, 0, f, G);
    if (rc) return rc;
    HIP_TRY(rtk::launch_denoise(f.mean, f.se, f.out, call.f64, p->width, p->height, p->radius, p->patch, p->k, G,
                                call.stream));
    rt_denoise_stats s{};
    s.radius = p->radius;
    s.patch = p->patch;
    s.lds_bytes = rtk::denoise_lds_bytes(p->radius, p->patch);
    return call.finish(c->flt_denoise, s);
}

// the guided filter with no guides
int rt_denoise(rt_ctx* c, const rt_denoise_params* p, const void* mean, const double* stderr_map, void* out)
{
    return rt_denoise_guided(c, p, mean, stderr_map, nullptr, out);
}

int rt_denoise_last_stats(rt_ctx* c, rt_denoise_stats* out) { return last_stats(c, &rt_ctx::flt_denoise, out); }

// ---- variance-guided a-trous wavelet filter (rt_abi.h: the filter; atrous_kernel.hip; atrous_host.cpp)
int rt_denoise_atrous(rt_ctx* c, const rt_atrous_params* p, const void* mean, const double* stderr_map,
                      const rt_denoise_guides* g, void* out, double* stderr_out)
{
    if (!c) return fail(RT_ERR_INVALID, "null argument");
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::atrous_check(p, mean, stderr_map, g, out, stderr_out, G)) return fail(RT_ERR_INVALID, bad);

    FilterCall call(c, *p);
    // the state scratch between levels (a call that needs none gets a null pointer)
    const size_t scratch_bytes = (size_t)rtk::atrous_state_buffers(p->levels) * call.hw * sizeof(rtk::AtrousRec);
    FilterFrames f{mean, nullptr, stderr_map, out, stderr_out};
    const int rc = call.begin(c->flt_atrous, scratch_bytes, f, G);
    if (rc) return rc;
    HIP_TRY(rtk::launch_atrous(f.mean, f.se, f.out, f.se_out, call.f64, p->width, p->height, p->levels, p->sigma_l,
                               p->demodulate ? G.albedo : nullptr, G, (rtk::AtrousRec*)call.scratch, call.stream));
    rt_atrous_stats s{};
    s.levels = p->levels;
    s.scratch_bytes = (int64_t)scratch_bytes;
    return call.finish(c->flt_atrous, s);
}

int rt_atrous_last_stats(rt_ctx* c, rt_atrous_stats* out) { return last_stats(c, &rt_ctx::flt_atrous, out); }

// ---- cross-filtered NL-means over two half frames (rt_abi.h: the filter; cross_kernel.hip; cross_host.cpp)
int rt_denoise_cross(rt_ctx* c, const rt_cross_params* p, const void* mean_a, const void* mean_b,
                     const double* stderr_map, const rt_denoise_guides* g, void* out, double* stderr_out)
{
    if (!c) return fail(RT_ERR_INVALID, "null argument");
    if (const char* bad = rtk::cross_check(p, mean_a, mean_b, stderr_map, out, stderr_out)) return fail(RT_ERR_INVALID, bad);
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::guides_check(g, G)) return fail(RT_ERR_INVALID, bad);

    FilterCall call(c, *p);
    // e(p) between the two kernels (a call without stderr_out needs none)
    const size_t scratch_bytes = stderr_out ? call.hw * sizeof(double) : 0;
    FilterFrames f{mean_a, mean_b, stderr_map, out, stderr_out};
    const int rc = call.begin(c->flt_cross, scratch_bytes, f, G);
    if (rc) return rc;
    HIP_TRY(rtk::launch_cross(f.mean, f.mean_b, f.se, f.out, f.se_out, (double*)call.scratch, call.f64, p->width,
                              p->height, p->radius, p->patch, p->k, p->variance_scale, G, call.stream));
    rt_cross_stats s{};
    s.radius = p->radius;
    s.patch = p->patch;
    s.lds_bytes = rtk::cross_lds_bytes(p->radius, p->patch);
    s.scratch_bytes = (int64_t)scratch_bytes;
    return call.finish(c->flt_cross, s);
}

int rt_cross_last_stats(rt_ctx* c, rt_cross_stats* out) { return last_stats(c, &rt_ctx::flt_cross, out); }

// ---- multi-scale NL-means (rt_abi.h: the filter; pyramid_kernel.hip; pyramid_host.cpp) ------------
int rt_denoise_pyramid(rt_ctx* c, const rt_pyramid_params* p, const void* mean, const double* stderr_map,
                       const rt_denoise_guides* g, void* out)
{
    if (!c) return fail(RT_ERR_INVALID, "null argument");
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::pyramid_check(p, mean, stderr_map, g, out, G)) return fail(RT_ERR_INVALID, bad);

    FilterCall call(c, *p);
    // the levels' f64 frames (a call of one level needs none and gets a null pointer)
    const rtk::PyramidLayout lay(p->width, p->height, p->levels, call.f64, G.albedo != nullptr, G.normal != nullptr,
                                 G.depth != nullptr);
    const size_t scratch_bytes = lay.doubles * sizeof(double);
    FilterFrames f{mean, nullptr, stderr_map, out, nullptr};
    const int rc = call.begin(c->flt_pyramid, scratch_bytes, f, G);
    if (rc) return rc;
    HIP_TRY(rtk::launch_pyramid(f.mean, f.se, f.out, call.f64, p->width, p->height, p->radius, p->patch, p->k, p->levels,
                                G, (double*)call.scratch, call.stream,
                                rtk::PyramidSide{c->tstream[0], c->ev_pf.ev[0], c->ev_pf.ev[1]}));
    rt_pyramid_stats s{};
    s.levels = p->levels;
    s.radius = p->radius;
    s.patch = p->patch;
    s.scratch_bytes = (int64_t)scratch_bytes;
    return call.finish(c->flt_pyramid, s);
}

int rt_pyramid_last_stats(rt_ctx* c, rt_pyramid_stats* out) { return last_stats(c, &rt_ctx::flt_pyramid, out); }

}  // extern "C"
