// abi_filters.cpp — the post-filters behind the C ABI (include/rt/rt_abi.h): the variance-guided
// NL-means filter (rt_denoise, rt_denoise_guided; denoise_kernel.hip), the variance-guided
// a-trous wavelet filter (rt_denoise_atrous; atrous_kernel.hip), the cross-filtered NL-means over
// two half frames (rt_denoise_cross; cross_kernel.hip) and the multi-scale NL-means
// (rt_denoise_pyramid; pyramid_kernel.hip), with their stats. Their host counterparts are
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
// pointers) their staged copies — the frame, the map, the result, the optional second result and
// the guides given.
struct FilterFrames {
    const void* mean;
    const double* se;
    void* out;
    double* se_out;
};

int stage_frames(HostStage& st, hipStream_t stream, size_t hw, size_t frame_bytes, FilterFrames& f, rtk::DenoiseGuides& G)
{
    const size_t b1 = hw * sizeof(double), b3 = 3 * b1;
    const int rc = st.stage(stream, {{f.mean, frame_bytes, false}, {f.se, b1, false}, {f.out, frame_bytes, true},
                                     {f.se_out, b1, true}, {G.albedo, b3, false}, {G.normal, b3, false},
                                     {G.depth, b1, false}});
    if (rc) return rc;
    f = FilterFrames{st.dev(0), (const double*)st.dev(1), st.dev(2), (double*)st.dev(3)};
    G.albedo = (const double*)st.dev(4);
    G.normal = (const double*)st.dev(5);
    G.depth = (const double*)st.dev(6);
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
    const bool f64 = p->format == RT_OUT_F64, on_dev = p->on_device != 0;
    const size_t hw = (size_t)p->width * (size_t)p->height;
    const size_t frame_bytes = hw * 3 * (f64 ? 8 : 4);

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;

    HostStage st;
    FilterFrames f{mean, stderr_map, out, nullptr};
    if (!on_dev) {
        rc = stage_frames(st, stream, hw, frame_bytes, f, G);
        if (rc) return rc;
    }
    HIP_TRY(c->ev_dn.record(0, stream));
    HIP_TRY(rtk::launch_denoise(f.mean, f.se, f.out, f64, p->width, p->height, p->radius, p->patch, p->k, G, stream));
    HIP_TRY(c->ev_dn.record(1, stream));
    c->dstats = rt_denoise_stats{};
    c->dstats.radius = p->radius;
    c->dstats.patch = p->patch;
    c->dstats.lds_bytes = rtk::denoise_lds_bytes(p->radius, p->patch);
    c->ev_dn.arm();
    rc = st.copy_back(stream);
    if (rc) return rc;
    rc = scope.end();
    if (rc) return rc;
    if (!on_dev) HIP_TRY(hipStreamSynchronize(stream));   // (the block is freed once its copies are done)
    return RT_OK;
}

// the guided filter with no guides
int rt_denoise(rt_ctx* c, const rt_denoise_params* p, const void* mean, const double* stderr_map, void* out)
{
    return rt_denoise_guided(c, p, mean, stderr_map, nullptr, out);
}

int rt_denoise_last_stats(rt_ctx* c, rt_denoise_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    if (c->ev_dn.pending) {
        HIP_TRY(hipSetDevice(c->device));
        float ms[1] = {0};
        const int rc = c->ev_dn.resolve(ms);
        if (rc) return rc;
        c->dstats.kernel_ms = ms[0];
    }
    *out = c->dstats;
    return RT_OK;
}

// ---- variance-guided a-trous wavelet filter (rt_abi.h: the filter; atrous_kernel.hip; atrous_host.cpp)
int rt_denoise_atrous(rt_ctx* c, const rt_atrous_params* p, const void* mean, const double* stderr_map,
                      const rt_denoise_guides* g, void* out, double* stderr_out)
{
    if (!c) return fail(RT_ERR_INVALID, "null argument");
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::atrous_check(p, mean, stderr_map, g, out, stderr_out, G)) return fail(RT_ERR_INVALID, bad);
    const bool f64 = p->format == RT_OUT_F64, on_dev = p->on_device != 0;
    const size_t hw = (size_t)p->width * (size_t)p->height;
    const size_t frame_bytes = hw * 3 * (f64 ? 8 : 4);
    const size_t scratch_bytes = (size_t)rtk::atrous_state_buffers(p->levels) * hw * sizeof(rtk::AtrousRec);

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;
    // the context's state scratch, grown on demand (a call that needs none gets a null pointer)
    rc = c->atrous_buf.reserve(stream, scratch_bytes);
    if (rc) return rc;
    rtk::AtrousRec* const scratch = scratch_bytes ? c->atrous_buf.as<rtk::AtrousRec>() : nullptr;

    HostStage st;
    FilterFrames f{mean, stderr_map, out, stderr_out};
    if (!on_dev) {
        rc = stage_frames(st, stream, hw, frame_bytes, f, G);
        if (rc) return rc;
    }
    HIP_TRY(c->ev_at.record(0, stream));
    HIP_TRY(rtk::launch_atrous(f.mean, f.se, f.out, f.se_out, f64, p->width, p->height, p->levels, p->sigma_l,
                               p->demodulate ? G.albedo : nullptr, G, scratch, stream));
    HIP_TRY(c->ev_at.record(1, stream));
    c->wstats = rt_atrous_stats{};
    c->wstats.levels = p->levels;
    c->wstats.scratch_bytes = (int64_t)scratch_bytes;
    c->ev_at.arm();
    rc = st.copy_back(stream);
    if (rc) return rc;
    rc = scope.end();
    if (rc) return rc;
    if (!on_dev) HIP_TRY(hipStreamSynchronize(stream));   // (the block is freed once its copies are done)
    return RT_OK;
}

int rt_atrous_last_stats(rt_ctx* c, rt_atrous_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    if (c->ev_at.pending) {
        HIP_TRY(hipSetDevice(c->device));
        float ms[1] = {0};
        const int rc = c->ev_at.resolve(ms);
        if (rc) return rc;
        c->wstats.kernel_ms = ms[0];
    }
    *out = c->wstats;
    return RT_OK;
}

// ---- cross-filtered NL-means over two half frames (rt_abi.h: the filter; cross_kernel.hip; cross_host.cpp)
int rt_denoise_cross(rt_ctx* c, const rt_cross_params* p, const void* mean_a, const void* mean_b,
                     const double* stderr_map, const rt_denoise_guides* g, void* out, double* stderr_out)
{
    if (!c) return fail(RT_ERR_INVALID, "null argument");
    if (const char* bad = rtk::cross_check(p, mean_a, mean_b, stderr_map, out, stderr_out)) return fail(RT_ERR_INVALID, bad);
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::guides_check(g, G)) return fail(RT_ERR_INVALID, bad);
    const bool f64 = p->format == RT_OUT_F64, on_dev = p->on_device != 0;
    const size_t hw = (size_t)p->width * (size_t)p->height;
    const size_t b1 = hw * sizeof(double), b3 = 3 * b1, frame_bytes = hw * 3 * (f64 ? 8 : 4);
    const size_t scratch_bytes = stderr_out ? b1 : 0;

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;
    // the context's e scratch, grown on demand (a call without stderr_out needs none)
    rc = c->cross_buf.reserve(stream, scratch_bytes);
    if (rc) return rc;
    double* const e = scratch_bytes ? c->cross_buf.as<double>() : nullptr;

    HostStage st;
    if (!on_dev) {
        rc = st.stage(stream, {{mean_a, frame_bytes, false}, {mean_b, frame_bytes, false}, {stderr_map, b1, false},
                               {out, frame_bytes, true}, {stderr_out, b1, true}, {G.albedo, b3, false},
                               {G.normal, b3, false}, {G.depth, b1, false}});
        if (rc) return rc;
        mean_a = st.dev(0);
        mean_b = st.dev(1);
        stderr_map = (const double*)st.dev(2);
        out = st.dev(3);
        stderr_out = (double*)st.dev(4);
        G.albedo = (const double*)st.dev(5);
        G.normal = (const double*)st.dev(6);
        G.depth = (const double*)st.dev(7);
    }
    HIP_TRY(c->ev_x.record(0, stream));
    HIP_TRY(rtk::launch_cross(mean_a, mean_b, stderr_map, out, stderr_out, e, f64, p->width, p->height, p->radius,
                              p->patch, p->k, p->variance_scale, G, stream));
    HIP_TRY(c->ev_x.record(1, stream));
    c->xstats = rt_cross_stats{};
    c->xstats.radius = p->radius;
    c->xstats.patch = p->patch;
    c->xstats.lds_bytes = rtk::cross_lds_bytes(p->radius, p->patch);
    c->xstats.scratch_bytes = (int64_t)scratch_bytes;
    c->ev_x.arm();
    rc = st.copy_back(stream);
    if (rc) return rc;
    rc = scope.end();
    if (rc) return rc;
    if (!on_dev) HIP_TRY(hipStreamSynchronize(stream));   // (the block is freed once its copies are done)
    return RT_OK;
}

int rt_cross_last_stats(rt_ctx* c, rt_cross_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    if (c->ev_x.pending) {
        HIP_TRY(hipSetDevice(c->device));
        float ms[1] = {0};
        const int rc = c->ev_x.resolve(ms);
        if (rc) return rc;
        c->xstats.kernel_ms = ms[0];
    }
    *out = c->xstats;
    return RT_OK;
}

// ---- multi-scale NL-means (rt_abi.h: the filter; pyramid_kernel.hip; pyramid_host.cpp) ------------
int rt_denoise_pyramid(rt_ctx* c, const rt_pyramid_params* p, const void* mean, const double* stderr_map,
                       const rt_denoise_guides* g, void* out)
{
    if (!c) return fail(RT_ERR_INVALID, "null argument");
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::pyramid_check(p, mean, stderr_map, g, out, G)) return fail(RT_ERR_INVALID, bad);
    const bool f64 = p->format == RT_OUT_F64, on_dev = p->on_device != 0;
    const size_t hw = (size_t)p->width * (size_t)p->height;
    const size_t frame_bytes = hw * 3 * (f64 ? 8 : 4);
    const rtk::PyramidLayout lay(p->width, p->height, p->levels, f64, G.albedo != nullptr, G.normal != nullptr,
                                 G.depth != nullptr);
    const size_t scratch_bytes = lay.doubles * sizeof(double);

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;
    // the context's level scratch, grown on demand (a call of one level needs none and gets a null pointer)
    rc = c->pyramid_buf.reserve(stream, scratch_bytes);
    if (rc) return rc;
    double* const scratch = scratch_bytes ? c->pyramid_buf.as<double>() : nullptr;

    HostStage st;
    FilterFrames f{mean, stderr_map, out, nullptr};
    if (!on_dev) {
        rc = stage_frames(st, stream, hw, frame_bytes, f, G);
        if (rc) return rc;
    }
    HIP_TRY(c->ev_py.record(0, stream));
    HIP_TRY(rtk::launch_pyramid(f.mean, f.se, f.out, f64, p->width, p->height, p->radius, p->patch, p->k, p->levels, G,
                                scratch, stream, rtk::PyramidSide{c->tstream[0], c->ev_pf.ev[0], c->ev_pf.ev[1]}));
    HIP_TRY(c->ev_py.record(1, stream));
    c->pstats = rt_pyramid_stats{};
    c->pstats.levels = p->levels;
    c->pstats.radius = p->radius;
    c->pstats.patch = p->patch;
    c->pstats.scratch_bytes = (int64_t)scratch_bytes;
    c->ev_py.arm();
    rc = st.copy_back(stream);
    if (rc) return rc;
    rc = scope.end();
    if (rc) return rc;
    if (!on_dev) HIP_TRY(hipStreamSynchronize(stream));   // (the block is freed once its copies are done)
    return RT_OK;
}

int rt_pyramid_last_stats(rt_ctx* c, rt_pyramid_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    if (c->ev_py.pending) {
        HIP_TRY(hipSetDevice(c->device));
        float ms[1] = {0};
        const int rc = c->ev_py.resolve(ms);
        if (rc) return rc;
        c->pstats.kernel_ms = ms[0];
    }
    *out = c->pstats;
    return RT_OK;
}

}  // extern "C"
