// ctx_internal.hpp — the private definition of a context (rt_ctx) and what every file behind the
// C ABI shares with it: the last-error helpers, the two owning types its device resources are kept
// in (DevBuf, EventSpan) and the cross-stream ordering scope. Not exported in include/rt/rt_abi.h.
// (What a render launches under the context's settings — the schedule AUTO resolves to, whether
// buffer batches overlap — is decided in launch_plan.cpp.)
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "rt/rt_abi.h"
#include "deal_cache.hpp"
#include "launch_plan.hpp"
#include "trace_kernel.hpp"

namespace rtx {

// rt_last_error's text for this thread (the one slot, abi.cpp); returns code
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

}  // namespace rtx

using rtx::fail;
using rtx::hip_fail;

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t e_ = (expr);                         \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

#pragma GCC visibility push(hidden)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// A device allocation and its capacity in bytes; freed when it goes out of scope.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;

    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }

    template <typename T>
    T* as() const { return (T*)p; }

    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    // a fresh allocation of `bytes` (whatever it held is freed first, unsynchronized: for a buffer
    // no enqueued work reads)
    hipError_t alloc(size_t bytes)
    {
        release();
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) p = nullptr;
        else cap = bytes;
        return e;
    }
    // Grown on demand: nothing if `bytes` fit, else `stream` is synchronized (the caller has
    // ordered it after every earlier use), the old buffer freed and the new one allocated — in
    // that order, so the peak is the larger of the two and not their sum. Out of device memory
    // with `oom` given: the buffer is left empty, *oom set and RT_ERR_HIP returned with the sticky
    // error cleared (the caller retries with less).
    int reserve(hipStream_t stream, size_t bytes, bool* oom = nullptr)
    {
        if (bytes <= cap) return RT_OK;
        HIP_TRY(hipStreamSynchronize(stream));
        const hipError_t e = alloc(bytes);
        if (e == hipErrorOutOfMemory && oom) {
            (void)hipGetLastError();
            *oom = true;
            return RT_ERR_HIP;
        }
        HIP_TRY(e);
        return RT_OK;
    }
};

// N events recorded along a stream now, read as N - 1 intervals in milliseconds later.
// (Created with hipEventDisableTiming and never armed: plain ordering events.)
template <int N>
struct EventSpan {
    hipEvent_t ev[N] = {};
    bool pending = false;   // recorded, its intervals not read yet

    EventSpan() = default;
    EventSpan(const EventSpan&) = delete;
    EventSpan& operator=(const EventSpan&) = delete;
    ~EventSpan()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }

    hipError_t create(unsigned flags = hipEventDefault)
    {
        hipError_t e = hipSuccess;
        for (int i = 0; i < N && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev[i], flags);
        return e;
    }
    hipError_t record(int i, hipStream_t stream) { return hipEventRecord(ev[i], stream); }
    hipError_t wait(int i) { return hipEventSynchronize(ev[i]); }
    // interval i: from event i to event i + 1, both complete
    hipError_t elapsed(int i, float* ms) { return hipEventElapsedTime(ms, ev[i], ev[i + 1]); }
    void arm() { pending = true; }
    void disarm() { pending = false; }
    // Nothing when not armed; else waits for the last event, reads the intervals and disarms.
    int resolve(float ms[N - 1])
    {
        if (!pending) return RT_OK;
        HIP_TRY(wait(N - 1));
        for (int i = 0; i + 1 < N; ++i) HIP_TRY(elapsed(i, &ms[i]));
        pending = false;
        return RT_OK;
    }
};

// What the context keeps for one post-filter (abi_filters.cpp): the last call's stats
// (rt_*_last_stats), the timing events around its kernels, and its scratch, grown on demand.
template <typename Stats>
struct FilterSlot {
    Stats stats{};
    EventSpan<2> ev;
    DevBuf scratch;
};

using rtk::kCounters;   // count_work counters (trace_kernel.hpp, CounterSlot; rt_last_counters)

struct rt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf scene_buf;                   // the uploaded scene's tables, one allocation
    rtk::SceneDev S{};
    bool has_scene = false;
    DevBuf partial;                     // the trace-output buffer (f64)
    DevBuf out_buf;                     // device staging for a host-bound result (never under 16 bytes)
    DevBuf counters;                    // kCounters x u64
    DevBuf params;                      // ring of kParamSlots device copies of the launch params (rtk::KParams)
    int param_slot = 0;
    EventSpan<3> ev;                    // a render: before its trace launches, after them, after its reductions
    // Cross-stream ordering: the scratch buffers (partial, work counter, acc_tmp, counters,
    // params ring, staging) are per context, so work enqueued on a new stream must wait for
    // everything the context enqueued on the previous one. ev_done is recorded after each
    // enqueue; a call on another stream first makes that stream wait for it.
    EventSpan<1> ev_done;
    hipStream_t last_stream = nullptr;
    bool any_enqueued = false;
    bool pending_counts = false;        // the render whose span is armed counted work (rt_last_stats, rt_last_tile_costs)
    rt_stats stats{};
    rt_adaptive_stats astats{};         // the last rt_render_adaptive (rt_adaptive_last_stats)
    FilterSlot<rt_denoise_stats> flt_denoise;   // rt_denoise, rt_denoise_guided: no scratch
    rt_features_stats fstats{};         // the last rt_render_features (rt_features_last_stats)
    EventSpan<3> ev_ft;                 //   before its trace launches, after them, after its reductions
    rt_query_stats qstats{};            // the last rt_trace_rays (rt_query_last_stats)
    EventSpan<2> ev_q;                  //   around a launch of trace_query
    DevBuf query_buf;                   //   a host-pointer call's device copies: a batch's rays, then its results
    FilterSlot<rt_atrous_stats> flt_atrous;     // rt_denoise_atrous: its state between levels (rtk::AtrousRec)
    FilterSlot<rt_cross_stats> flt_cross;       // rt_denoise_cross: e(p) between its two kernels (f64 per pixel; only with stderr_out)
    FilterSlot<rt_pyramid_stats> flt_pyramid;   // rt_denoise_pyramid: its levels' f64 frames (rtk::PyramidLayout; none at one level)
    EventSpan<2> ev_pf;                 //   fork and join of the pyramid's coarse levels' filters on tstream[0] (ordering events)
    // what a render's launch plan is made from (launch_plan.hpp): the uploaded scene, the device, the switches
    rtp::SceneFacts scene;
    rtp::DeviceFacts dev;
    rtp::Options opt;
    int opt_comm_direct = 1;            // RT_OPT_COMM_DIRECT: a world-1 rt_render_gather renders straight into the frame
    DevBuf ring;                        // RT_OPT_POOL_RING's per-wave record rings (kPoolRing blocks per wave; f64)
    unsigned long long raw_counters[kCounters] = {};   // the last count_work render's counters (rt_last_counters)
    DevBuf tile_order;                  // rt_ctx_set_tile_order: tile shards' position -> raster tile (u32)
    int64_t tile_order_n = 0;           //   its length (0: raster order)
    DevBuf tile_cost;                   // count_work pool renders: lane-cycles per raster tile (u64)
    int64_t tile_cost_n = 0;            //   tiles of the last count_work render (rt_last_tile_costs)
    int opt_hoist = 1;                  // RT_OPT_HOIST: test a huge root-child leaf before the walk (pre_leaf)
    size_t sample_buf_cap = (size_t)32 << 30;  // RT_OPT_TRACE_BUF_BYTES: bound of the trace-output buffer
    DevBuf work;                        // pool / item schedules: work-block counters (u32; one per overlapped batch),
    size_t work_stride = rtk::kDealTable;   //   work_stride words apart: each one's deal table and tile costs follow it
    // Overlapped buffer batches (RT_OPT_BATCH_OVERLAP): batch k traces on tstream[k & 1] into half k & 1
    // of the trace-output buffer while the caller's stream reduces batch k - 1
    hipStream_t tstream[2] = {nullptr, nullptr};
    EventSpan<1> ev_in;
    EventSpan<2> ev_tr, ev_rd;
    DevBuf acc_tmp;                     // running sums when a render takes several buffer batches (f64)
    // RT_OPT_AUTO_DEAL_ORDER (deal_cache.hpp): whole-frame pool renders dealt in the cost order the
    // product kernel measured on the first render of a (scene upload, camera, frame)
    int opt_deal = rtd::kAuto;
    uint64_t upload_gen = 0;            // scene uploads so far (the cache's key)
    rtd::DealCache deal;
    int64_t deal_cap = 0;               // tiles the deal tables behind the work counters hold (trace_kernel.hpp, kDealTable)
    int64_t last_deal_n = 0;            // tiles of the order the last render was dealt in (0: raster; rt_last_deal_order)
    // RT_OPT_PRIMARY_CANDIDATES (primary_candidates.hpp): the candidate table of the (scene upload, camera,
    // frame size) it was last built for, kept beside the deal cache's key and dropped with it
    int opt_primary = 1;                // the option (0: every primary ray walks)
    int opt_primary_k = 7;              // RT_OPT_PRIMARY_CANDIDATES_K: candidates before a pixel is flagged (tests force 1)
    DevBuf primary_tab;                 // width x height 16-byte records, then one u32: the pixels flagged "walk"
    bool primary_valid = false;
    rtd::Key primary_key;               //   (the row-shard geometry left at its defaults: the table is the frame's)
    int primary_k = 0;                  //   the k it was built with
    int64_t primary_flagged = 0;        //   its flagged pixels
    EventSpan<2> ev_pc;                 //   around its build
    // RT_OPT_SKIP_SKY_TILES: the table's all-sky tiles, built, cached and dropped with it
    int opt_sky = 1;                    // the option (0: every tile is traced)
    int opt_defer_roots = 1;            // RT_OPT_DEFER_ROOTS (0: the primary-candidate kernel computes every candidate's exact root)
    DevBuf sky_tab;                     // one u32 (how many are set), 12 bytes unused, then a flag byte per raster tile
    std::vector<uint8_t> sky_flags;     //   the host's copy of the flags (the deal tables are filtered with it)
    int64_t sky_n = 0;                  //   how many are set
    uint64_t sky_gen = 0;               //   counts the builds (from 1)
    uint64_t deal_sky_gen = 0;          // the build whose flagged tiles the device's deal tables leave out (0: they list every tile)
    uint8_t* sky_dev() const { return reinterpret_cast<uint8_t*>(sky_tab.p) + 16; }
};

// Orders what a call enqueues on `stream` after everything this context enqueued on another
// stream before (its scratch buffers are shared between its renders): begin() ... end() around
// every call that enqueues. Once begin() has run, end() runs on every way out, an early error
// return included — work already queued on `stream` before the error still reads the context's
// buffers, and the next call on another stream must wait for it (ev_done, last_stream), not for
// the call before.
struct StreamScope {
    rt_ctx* c;
    hipStream_t stream;
    bool open = false;
    StreamScope(rt_ctx* c_, hipStream_t s_) : c(c_), stream(s_) {}
    int begin()
    {
        if (c->any_enqueued && stream != c->last_stream) HIP_TRY(hipStreamWaitEvent(stream, c->ev_done.ev[0], 0));
        open = true;
        return RT_OK;
    }
    int end()
    {
        open = false;
        HIP_TRY(c->ev_done.record(0, stream));
        c->last_stream = stream;
        c->any_enqueued = true;
        return RT_OK;
    }
    ~StreamScope()
    {
        if (open) (void)end();
    }
};

#pragma GCC visibility pop
