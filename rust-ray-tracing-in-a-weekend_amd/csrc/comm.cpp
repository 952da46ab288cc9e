// comm.cpp — the multi-GPU render behind the C ABI (rt_abi.h, "multi-GPU render"; ABI v5).
//
// The reference splits one frame over 10 std::threads, each tracing every pixel with spp/10
// samples into its own buffer, and sums the buffers under a mutex (main.rs:497-551, merge at
// :542-547). Here the split is over GPUs and by image area: rank r of `world` renders the 8x8
// tiles at positions r, r + world, ... of the frame's tile order (one slab per rank, rt_render's
// tile_shard layout), one RCCL gather moves the slabs to rank 0 over xGMI, and a reorder kernel
// (trace_kernel.hip, assemble_tiles) writes the frame there. Every draw is keyed by (pixel,
// sample), so the frame equals rt_render's bit for bit at any world size or tile order (in the
// f32 mode: whenever the shards and the whole frame run the same trace kernel, rt_abi.h). What a
// rank sends and where it lands on rank 0 is stated once, in comm_layout.hpp.
//
// RCCL is loaded with dlopen when the first communicator is made (librccl.so.1: the process's
// copy if one is loaded already — torch's, say — else the ROCm install's), so the library and
// every single-GPU entry point load and run without it.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <vector>

#include "comm_layout.hpp"
#include "ctx_internal.hpp"
#include "deal_cache.hpp"
#include "rt/rt_abi.h"
#include "trace_kernel.hpp"

namespace {

// ---- RCCL, resolved at run time ------------------------------------------------------------------
struct Rccl {
    void* h = nullptr;
    std::string err;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGather) Gather = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};

const Rccl& rccl()
{
    static Rccl R;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* name : {"librccl.so.1", "/opt/rocm/lib/librccl.so.1"}) {
            R.h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (R.h) break;
            const char* e = dlerror();
            R.err = e ? e : "dlopen failed";
        }
        if (!R.h) return;
        bool ok = true;
        auto sym = [&](auto& fn, const char* name) {
            fn = reinterpret_cast<std::remove_reference_t<decltype(fn)>>(dlsym(R.h, name));
            if (!fn) {
                ok = false;
                R.err = std::string("librccl.so.1 has no ") + name;
            }
        };
        sym(R.GetUniqueId, "ncclGetUniqueId");
        sym(R.CommInitRank, "ncclCommInitRank");
        sym(R.CommInitAll, "ncclCommInitAll");
        sym(R.CommDestroy, "ncclCommDestroy");
        sym(R.Gather, "ncclGather");
        sym(R.AllReduce, "ncclAllReduce");
        sym(R.GroupStart, "ncclGroupStart");
        sym(R.GroupEnd, "ncclGroupEnd");
        sym(R.GetErrorString, "ncclGetErrorString");
        if (!ok) R.h = nullptr;
    });
    return R;
}

int load_rccl(const Rccl*& R)
{
    R = &rccl();
    if (!R->h) return fail(RT_ERR_COMM, "RCCL not available: " + R->err);
    return RT_OK;
}

int nccl_fail(const Rccl& R, ncclResult_t r, const char* what)
{
    return fail(RT_ERR_COMM, std::string(what) + ": " + (R.GetErrorString ? R.GetErrorString(r) : "RCCL error"));
}

#define NCCL_TRY(R, expr)                                              \
    do {                                                               \
        ncclResult_t r_ = (expr);                                      \
        if (r_ != ncclSuccess) return nccl_fail((R), r_, #expr);       \
    } while (0)

}  // namespace

struct rt_comm {
    rt_ctx* ctx = nullptr;
    int rank = 0, world = 1, device = 0;
    ncclComm_t nc = nullptr;
    // this rank's tile slab (+ an 8-byte status trailer, sent with it), rank 0's gathered slabs,
    // rank 0's frame for a host-bound result, and the tile-cost vector of rt_comm_tile_order
    DevBuf slab, recv, stage, cost;   // (grown on demand, after the stream's earlier frames: no one still reads them)
    EventSpan<4> ev;            // render start / end, gathered, assembled; armed: a gather's events not yet read into stats
    rt_comm_stats stats{};
    bool direct = false;        // the last frame was a world-1 direct render (no slabs gathered)
    rtc::SlabLayout lay;        // the last gathered frame's slabs (rank 0: where the peers' status trailers lie in recv)
};

namespace {

bool bad_frame(const rt_render_params* p)
{
    return !p || p->width < 2 || p->height < 2 || p->spp < 1 || p->max_depth < 0 ||
           (p->out_format != RT_OUT_F32 && p->out_format != RT_OUT_F64) ||
           (long long)p->width * p->height > 0xffffffffLL;
}

// One frame's shard on one rank: the render params of its tile shard and the slab geometry
// (comm_layout.hpp: every rank's slab is padded to the largest shard's, rank 0's; + the status trailer).
struct Shard {
    rt_render_params q;
    rtc::SlabLayout lay;
};

// Every rank computes the same frame geometry from the same p, and a collective call sets the same
// tile order on every rank's context (rt_comm_tile_order; rt_ctx_set_tile_order is the caller's to
// keep alike), so what fails here fails on every rank alike, before any of them enqueued anything.
int shard_of(const rt_comm* m, const rt_render_params* p, hipStream_t s, Shard& f)
{
    if (bad_frame(p)) return fail(RT_ERR_INVALID, "bad render params");
    f.q = *p;
    f.q.row_block = 0;
    f.q.tile_shard = 1;
    f.q.row_begin = m->rank;
    f.q.row_stride = m->world;
    f.q.out_on_device = 1;
    f.q.stream = s;
    f.lay = rtc::slab_layout(p->width, p->height, m->rank, m->world, p->out_format == RT_OUT_F64 ? 8 : 4);
    if (f.lay.n_max <= 0) return fail(RT_ERR_INVALID, "frame too large for a tile shard");
    // a tile order made for another frame: the shard render would refuse it, but the reorder kernel
    // reads order[pos] for every tile position of this frame (rt_tiles_assemble refuses it alike)
    const int64_t n_order = m->ctx->tile_order_n;
    const int64_t n_tiles = (int64_t)((p->width + 7) / 8) * ((p->height + 7) / 8);
    if (n_order > 0 && n_order != n_tiles) return fail(RT_ERR_INVALID, "the context's tile order is for another frame");
    return RT_OK;
}

hipStream_t stream_of(const rt_comm* m, const rt_render_params* p)
{
    return p && p->stream ? (hipStream_t)p->stream : m->ctx->stream;
}

// Renders this rank's shard into its slab and writes the status trailer (0, or -rc when the
// render could not be enqueued: the rank still takes part in the gather, so no peer waits
// forever, and rank 0 sees the failure in the trailer). Returns the render's rc.
int enqueue_shard(rt_comm* m, const rt_camera* cam, const Shard& f, hipStream_t s)
{
    HIP_TRY(hipSetDevice(m->device));
    int rc = m->slab.reserve(s, f.lay.slab_bytes);
    if (rc) return rc;
    if (m->rank == 0) {
        rc = m->recv.reserve(s, f.lay.gathered_bytes());
        if (rc) return rc;
    }
    HIP_TRY(m->ev.record(0, s));
    rc = rt_render(m->ctx, cam, &f.q, m->slab.p);
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(m->ev.record(1, s));
    static_assert(rtc::kTrailerBytes == 2 * sizeof(int32_t), "the trailer is written as two words");
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(m->slab.as<char>() + f.lay.status_off()), rtc::status_of(rc), 2, s));
    m->lay = f.lay;
    return rc;
}

int enqueue_gather(const Rccl& R, rt_comm* m, const Shard& f, hipStream_t s)
{
    NCCL_TRY(R, R.Gather(m->slab.p, m->rank == 0 ? m->recv.p : nullptr, f.lay.slab_bytes, ncclUint8, 0, m->nc, s));
    HIP_TRY(m->ev.record(2, s));
    return RT_OK;
}

// Rank 0: the reorder kernel into the frame (the caller's device buffer, or the staging buffer
// copied to the caller's host memory), in the context's tile order.
int enqueue_assemble(rt_comm* m, const rt_render_params* p, const Shard& f, hipStream_t s, void* frame)
{
    const size_t frame_bytes = (size_t)p->width * p->height * 3 * f.lay.esz;
    void* dst = frame;
    if (!p->out_on_device) {
        const int rc = m->stage.reserve(s, frame_bytes);
        if (rc) return rc;
        dst = m->stage.p;
    }
    HIP_TRY(rtk::launch_assemble_tiles(m->recv.p, dst, f.lay.esz == 8, m->world, f.lay.stride_elems(),
                                       p->width, p->height, m->ctx->tile_order.as<uint32_t>(), s));
    HIP_TRY(m->ev.record(3, s));
    if (!p->out_on_device) HIP_TRY(hipMemcpyAsync(frame, dst, frame_bytes, hipMemcpyDeviceToHost, s));
    return RT_OK;
}

// Rank 0 once the gather has completed: the ranks' status trailers, read from the gathered slabs.
int scan_peers(rt_comm* m, rtc::StatusScan& scan)
{
    std::vector<int32_t> st((size_t)m->world, 0);
    for (int r = 0; r < m->world; ++r)
        HIP_TRY(hipMemcpy(&st[(size_t)r], m->recv.as<char>() + m->lay.status_at(r), sizeof(int32_t), hipMemcpyDeviceToHost));
    scan = rtc::scan_status(st.data(), m->world);
    return RT_OK;
}

// Rank 0 after its stream is synchronized: RT_ERR_PEER if any rank's shard render failed.
int peer_status(rt_comm* m)
{
    rtc::StatusScan scan;
    const int rc = scan_peers(m, scan);
    if (rc) return rc;
    if (scan.failed)
        return fail(RT_ERR_PEER, "rank " + std::to_string(scan.first) + "'s shard render failed (" +
                                     std::to_string(scan.first_rc) + "): the frame is incomplete");
    return RT_OK;
}

void note_gather(rt_comm* m, const Shard& f)
{
    m->ev.arm();
    m->direct = false;
    m->stats.slab_bytes = (int64_t)f.lay.slab_bytes;
    m->stats.tiles = f.lay.n_mine;
}

// A world of one (RT_OPT_COMM_DIRECT, raster tile order): rt_render straight into the frame.
// The frame is the tile path's bit for bit (every draw keyed by (pixel, sample)); it skips the
// slab, the one-rank gather and the reorder pass (C2 at N = 1: 75.09 -> 74.70-74.92 ms per step,
// profiles/r06e_c2_*.log). The stats' gather and assemble times are 0.
bool direct_ok(const rt_comm* m)
{
    return m->world == 1 && m->ctx->tile_order_n == 0 && m->ctx->opt_comm_direct != 0;
}

int render_direct(rt_comm* m, const rt_camera* cam, const rt_render_params* p, hipStream_t s, void* frame)
{
    if (bad_frame(p)) return fail(RT_ERR_INVALID, "bad render params");
    rt_render_params q = *p;
    q.row_begin = 0;
    q.row_stride = 1;
    q.row_block = 0;
    q.tile_shard = 0;
    q.stream = s;
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(m->ev.record(0, s));
    const int rc = rt_render(m->ctx, cam, &q, frame);
    HIP_TRY(hipSetDevice(m->device));
    for (int i = 1; i < 4; ++i) HIP_TRY(m->ev.record(i, s));
    m->ev.arm();
    m->direct = true;
    m->stats.slab_bytes = 0;
    m->stats.tiles = rt_tiles_in_shard(p->width, p->height, 0, 1);
    return rc;
}

int check_comms(rt_comm* const* comms, int n)
{
    if (!comms || n < 1) return fail(RT_ERR_INVALID, "no communicators");
    for (int i = 0; i < n; ++i)
        if (!comms[i] || comms[i]->rank != i || comms[i]->world != n)
            return fail(RT_ERR_INVALID, "comms[i] must be rank i of a world of n (rt_comm_init_all)");
    return RT_OK;
}

// ---- rt_comm_tile_order's phases -------------------------------------------------------------------
struct CostPass {
    int rc = RT_OK;
    int schedule = RT_SCHED_AUTO, precision = RT_PREC_F64;
    int64_t n_tiles = 0;
    std::chrono::steady_clock::time_point t0;
};

// The count pass of this rank's raster shard, its tile costs (+ a failure flag) into m->cost.
// Returns an error only when the all-reduce could not be fed (then the caller must not enter it:
// the peers see no contribution... which RCCL cannot express, so this is limited to argument
// errors every rank shares).
int cost_local(rt_comm* m, const rt_camera* cam, const rt_render_params* p, int cost_spp, hipStream_t s, CostPass& cp)
{
    cp.t0 = std::chrono::steady_clock::now();
    if (bad_frame(p) || cost_spp < 1) return fail(RT_ERR_INVALID, "bad render params or cost_spp");
    cp.n_tiles = (int64_t)((p->width + 7) / 8) * ((p->height + 7) / 8);
    HIP_TRY(hipSetDevice(m->device));
    int rc = m->cost.reserve(s, (size_t)(cp.n_tiles + 1) * sizeof(uint64_t));
    if (rc) return rc;
    cp.schedule = m->ctx->opt.schedule;
    cp.precision = m->ctx->opt.precision;
    std::vector<uint64_t> h((size_t)cp.n_tiles + 1, 0);
    // raster shards, f64 (count_work's tile costs), a pool schedule (the chunk schedule counts none)
    rc = rt_ctx_set_tile_order(m->ctx, nullptr, 0);
    if (!rc && cp.precision != RT_PREC_F64) rc = rt_ctx_set_precision(m->ctx, RT_PREC_F64);
    if (!rc && cp.schedule == RT_SCHED_CHUNKS) rc = rt_ctx_set_schedule(m->ctx, RT_SCHED_POOL);
    Shard f;
    rt_render_params q = *p;
    q.spp = cost_spp;
    q.count_work = 1;
    q.out_format = RT_OUT_F32;
    if (!rc) rc = shard_of(m, &q, s, f);
    if (!rc) rc = m->slab.reserve(s, f.lay.slab_bytes);
    if (!rc) rc = rt_render(m->ctx, cam, &f.q, m->slab.p);
    if (!rc) {
        const int got = rt_last_tile_costs(m->ctx, h.data(), cp.n_tiles);   // synchronizes the render
        if (got < 0) rc = got;
        else if (got != cp.n_tiles) rc = fail(RT_ERR_UNSUPPORTED, "the count pass recorded no tile costs");
    }
    (void)rt_ctx_set_precision(m->ctx, cp.precision);
    (void)rt_ctx_set_schedule(m->ctx, cp.schedule);
    cp.rc = rc;
    if (rc) std::fill(h.begin(), h.end(), 0);
    h[(size_t)cp.n_tiles] = rc ? 1 : 0;   // failures, summed over the ranks
    HIP_TRY(hipSetDevice(m->device));
    HIP_TRY(hipMemcpyAsync(m->cost.p, h.data(), h.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));   // (h is pageable and local)
    return RT_OK;
}

int cost_finish(rt_comm* m, hipStream_t s, CostPass& cp)
{
    HIP_TRY(hipSetDevice(m->device));
    std::vector<uint64_t> h((size_t)cp.n_tiles + 1, 0);
    HIP_TRY(hipMemcpyAsync(h.data(), m->cost.p, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int rc = RT_OK;
    if (h[(size_t)cp.n_tiles] != 0) {   // some rank's pass failed: every rank keeps raster order
        (void)rt_ctx_set_tile_order(m->ctx, nullptr, 0);
        rc = cp.rc ? cp.rc : fail(RT_ERR_PEER, "another rank's cost pass failed: raster tile order");
        m->stats.tile_order = 0;
    } else {
        std::vector<uint32_t> order((size_t)cp.n_tiles);
        rc = rt_cost_tile_order(h.data(), cp.n_tiles, order.data());
        if (!rc) rc = rt_ctx_set_tile_order(m->ctx, order.data(), cp.n_tiles);
        m->stats.tile_order = rc ? 0 : 1;
    }
    m->stats.cost_pass_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - cp.t0).count();
    return rc;
}

}  // namespace

extern "C" {

int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES])
{
    if (!id) return fail(RT_ERR_INVALID, "null id");
    const Rccl* R;
    int rc = load_rccl(R);
    if (rc) return rc;
    ncclUniqueId u;
    NCCL_TRY(*R, R->GetUniqueId(&u));
    static_assert(sizeof u == RT_COMM_ID_BYTES, "ncclUniqueId size");
    std::memcpy(id, &u, sizeof u);
    return RT_OK;
}

static int comm_new(rt_ctx* ctx, int rank, int world, rt_comm** out)
{
    rt_comm* m = new (std::nothrow) rt_comm();
    if (!m) return fail(RT_ERR_OOM, "rt_comm");
    m->ctx = ctx;
    m->rank = rank;
    m->world = world;
    m->device = ctx->device;
    hipError_t e = hipSetDevice(m->device);
    if (e == hipSuccess) e = m->ev.create();
    if (e != hipSuccess) {
        delete m;
        return hip_fail(e, "rt_comm events");
    }
    *out = m;
    return RT_OK;
}

int rt_comm_init_rank(rt_ctx* ctx, int rank, int world, const uint8_t id[RT_COMM_ID_BYTES], rt_comm** out)
{
    if (!ctx || !id || !out || world < 1 || rank < 0 || rank >= world) return fail(RT_ERR_INVALID, "bad argument");
    *out = nullptr;
    const Rccl* R;
    int rc = load_rccl(R);
    if (rc) return rc;
    rt_comm* m = nullptr;
    rc = comm_new(ctx, rank, world, &m);
    if (rc) return rc;
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof u);
    const ncclResult_t r = R->CommInitRank(&m->nc, world, u, rank);
    if (r != ncclSuccess) {
        rt_comm_destroy(m);
        return nccl_fail(*R, r, "ncclCommInitRank");
    }
    *out = m;
    return RT_OK;
}

int rt_comm_init_all(rt_ctx* const* ctxs, int n, rt_comm** comms_out)
{
    if (!ctxs || !comms_out || n < 1) return fail(RT_ERR_INVALID, "bad argument");
    const Rccl* R;
    int rc = load_rccl(R);
    if (rc) return rc;
    std::vector<int> dev((size_t)n);
    for (int i = 0; i < n; ++i) {
        comms_out[i] = nullptr;
        if (!ctxs[i]) return fail(RT_ERR_INVALID, "null context");
        dev[(size_t)i] = ctxs[i]->device;
        for (int j = 0; j < i; ++j)
            if (dev[(size_t)j] == dev[(size_t)i]) return fail(RT_ERR_INVALID, "two contexts on one device");
    }
    std::vector<ncclComm_t> nc((size_t)n, nullptr);
    NCCL_TRY(*R, R->CommInitAll(nc.data(), n, dev.data()));
    for (int i = 0; i < n; ++i) {
        rc = comm_new(ctxs[i], i, n, &comms_out[i]);
        if (rc) {
            for (int j = 0; j < n; ++j) {
                if (comms_out[j]) rt_comm_destroy(comms_out[j]);
                else if (nc[(size_t)j]) (void)R->CommDestroy(nc[(size_t)j]);
                comms_out[j] = nullptr;
            }
            return rc;
        }
        comms_out[i]->nc = nc[(size_t)i];
    }
    return RT_OK;
}

void rt_comm_destroy(rt_comm* m)
{
    if (!m) return;
    (void)hipSetDevice(m->device);
    for (int i = 0; i < 4; ++i)
        if (m->ev.ev[i]) (void)m->ev.wait(i);
    (void)hipStreamSynchronize(m->ctx->stream);
    if (m->nc) {
        const Rccl& R = rccl();
        if (R.CommDestroy) (void)R.CommDestroy(m->nc);
    }
    delete m;   // (the buffers and events free themselves)
}

int rt_comm_rank(const rt_comm* m, int* rank, int* world)
{
    if (!m) return fail(RT_ERR_INVALID, "null communicator");
    if (rank) *rank = m->rank;
    if (world) *world = m->world;
    return RT_OK;
}

int rt_comm_tile_order(rt_comm* m, const rt_camera* cam, const rt_render_params* p, int cost_spp)
{
    if (!m || !cam || !p) return fail(RT_ERR_INVALID, "null argument");
    const Rccl* R;
    int rc = load_rccl(R);
    if (rc) return rc;
    const hipStream_t s = stream_of(m, p);
    CostPass cp;
    rc = cost_local(m, cam, p, cost_spp, s, cp);
    if (rc) return rc;
    NCCL_TRY(*R, R->AllReduce(m->cost.p, m->cost.p, (size_t)cp.n_tiles + 1, ncclUint64, ncclSum, m->nc, s));
    return cost_finish(m, s, cp);
}

int rt_comm_tile_order_all(rt_comm* const* comms, int n, const rt_camera* cam, const rt_render_params* p,
                           int cost_spp)
{
    int rc = check_comms(comms, n);
    if (rc) return rc;
    if (!cam || !p) return fail(RT_ERR_INVALID, "null argument");
    if (p->stream) return fail(RT_ERR_INVALID, "the *_all calls run on each context's stream: p->stream must be NULL");
    const Rccl* R;
    rc = load_rccl(R);
    if (rc) return rc;
    std::vector<CostPass> cp((size_t)n);
    for (int i = 0; i < n; ++i) {
        rc = cost_local(comms[i], cam, p, cost_spp, comms[i]->ctx->stream, cp[(size_t)i]);
        if (rc) return rc;
    }
    NCCL_TRY(*R, R->GroupStart());
    for (int i = 0; i < n; ++i) {
        rt_comm* m = comms[i];
        const ncclResult_t r = R->AllReduce(m->cost.p, m->cost.p, (size_t)cp[(size_t)i].n_tiles + 1, ncclUint64, ncclSum,
                                            m->nc, m->ctx->stream);
        if (r != ncclSuccess) {
            (void)R->GroupEnd();
            return nccl_fail(*R, r, "ncclAllReduce");
        }
    }
    NCCL_TRY(*R, R->GroupEnd());
    int first = RT_OK;
    for (int i = 0; i < n; ++i) {
        rc = cost_finish(comms[i], comms[i]->ctx->stream, cp[(size_t)i]);
        if (rc && !first) first = rc;
    }
    return first;
}

int rt_render_gather(rt_comm* m, const rt_camera* cam, const rt_render_params* p, void* frame)
{
    if (!m || !cam || !p) return fail(RT_ERR_INVALID, "null argument");
    if (m->rank == 0 && !frame) return fail(RT_ERR_INVALID, "rank 0 needs a frame");
    if (direct_ok(m)) return render_direct(m, cam, p, stream_of(m, p), frame);
    const Rccl* R;
    int rc = load_rccl(R);
    if (rc) return rc;
    const hipStream_t s = stream_of(m, p);
    Shard f;
    rc = shard_of(m, p, s, f);   // (argument errors: every rank has the same p and fails alike)
    if (rc) return rc;
    const int rc_render = enqueue_shard(m, cam, f, s);
    if (m->slab.cap < f.lay.slab_bytes || (m->rank == 0 && m->recv.cap < f.lay.gathered_bytes()))
        return rc_render;   // no buffers to send from: this rank stays out of the gather (its peers may
                            // already have enqueued theirs, and then wait for it: DESIGN.md, known gaps)
    rc = enqueue_gather(*R, m, f, s);
    if (rc) return rc;
    note_gather(m, f);
    if (m->rank == 0) {
        rc = enqueue_assemble(m, p, f, s, frame);
        if (rc) return rc;
    }
    if (p->out_on_device) return rc_render;
    HIP_TRY(hipStreamSynchronize(s));
    if (rc_render) return rc_render;
    return m->rank == 0 ? peer_status(m) : RT_OK;
}

int rt_render_gather_all(rt_comm* const* comms, int n, const rt_camera* cam, const rt_render_params* p, void* frame)
{
    int rc = check_comms(comms, n);
    if (rc) return rc;
    if (!cam || !p || !frame) return fail(RT_ERR_INVALID, "null argument");
    if (p->stream) return fail(RT_ERR_INVALID, "the *_all calls run on each context's stream: p->stream must be NULL");
    const Rccl* R;
    rc = load_rccl(R);
    if (rc) return rc;
    if (n == 1 && direct_ok(comms[0])) return render_direct(comms[0], cam, p, comms[0]->ctx->stream, frame);
    std::vector<Shard> f((size_t)n);
    for (int i = 0; i < n; ++i) {
        rc = shard_of(comms[i], p, comms[i]->ctx->stream, f[(size_t)i]);
        if (rc) return rc;
    }
    int rc_render = RT_OK;
    for (int i = 0; i < n; ++i) {   // every render enqueued before any gather: the GPUs trace at once
        rc = enqueue_shard(comms[i], cam, f[(size_t)i], comms[i]->ctx->stream);
        if (rc && !rc_render) rc_render = rc;
        if (comms[i]->slab.cap < f[(size_t)i].lay.slab_bytes ||
            (i == 0 && comms[0]->recv.cap < f[0].lay.gathered_bytes()))
            return rc;   // no buffers: nothing to gather
    }
    NCCL_TRY(*R, R->GroupStart());
    for (int i = 0; i < n; ++i) {
        rt_comm* m = comms[i];
        const ncclResult_t r = R->Gather(m->slab.p, i == 0 ? m->recv.p : nullptr, f[(size_t)i].lay.slab_bytes, ncclUint8, 0,
                                         m->nc, m->ctx->stream);
        if (r != ncclSuccess) {
            (void)R->GroupEnd();
            return nccl_fail(*R, r, "ncclGather");
        }
    }
    NCCL_TRY(*R, R->GroupEnd());
    for (int i = 0; i < n; ++i) {
        HIP_TRY(hipSetDevice(comms[i]->device));
        HIP_TRY(comms[i]->ev.record(2, comms[i]->ctx->stream));
        note_gather(comms[i], f[(size_t)i]);
    }
    HIP_TRY(hipSetDevice(comms[0]->device));
    rc = enqueue_assemble(comms[0], p, f[0], comms[0]->ctx->stream, frame);
    if (rc) return rc;
    if (p->out_on_device) return rc_render;
    for (int i = 0; i < n; ++i) {
        HIP_TRY(hipSetDevice(comms[i]->device));
        HIP_TRY(hipStreamSynchronize(comms[i]->ctx->stream));
    }
    if (rc_render) return rc_render;
    HIP_TRY(hipSetDevice(comms[0]->device));
    return peer_status(comms[0]);
}

int rt_comm_last_stats(rt_comm* m, rt_comm_stats* out)
{
    if (!m || !out) return fail(RT_ERR_INVALID, "null argument");
    if (m->ev.pending) {   // (not resolve(): only rank 0 records the last event)
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(m->ev.wait(2));
        float a = 0, b = 0, c = 0;
        HIP_TRY(m->ev.elapsed(0, &a));
        HIP_TRY(m->ev.elapsed(1, &b));
        if (m->rank == 0) {
            HIP_TRY(m->ev.wait(3));
            HIP_TRY(m->ev.elapsed(2, &c));
        }
        m->stats.render_ms = a;
        m->stats.gather_ms = b;
        m->stats.assemble_ms = c;
        rt_stats st;
        if (rt_last_stats(m->ctx, &st) == RT_OK) m->stats.kernel_ms = st.kernel_ms;
        m->stats.peer_failed = 0;
        if (m->rank == 0 && !m->direct) {
            rtc::StatusScan scan;
            const int rc = scan_peers(m, scan);
            if (rc) return rc;
            m->stats.peer_failed = scan.failed;
        }
        m->ev.disarm();
    }
    *out = m->stats;
    return RT_OK;
}

int rt_tiles_assemble(rt_ctx* ctx, const void* slabs, int64_t slab_elems, int world, const rt_render_params* p,
                      void* frame)
{
    if (!ctx || !slabs || !frame || world < 1 || bad_frame(p)) return fail(RT_ERR_INVALID, "bad argument");
    const rtc::SlabLayout lay = rtc::slab_layout(p->width, p->height, 0, world, p->out_format == RT_OUT_F64 ? 8 : 4);
    if (lay.n_max <= 0 || slab_elems < lay.slab_elems) return fail(RT_ERR_INVALID, "slab_elems below the largest shard's");
    const int64_t n_order = ctx->tile_order_n;
    const int64_t n_tiles = (int64_t)((p->width + 7) / 8) * ((p->height + 7) / 8);
    if (n_order > 0 && n_order != n_tiles) return fail(RT_ERR_INVALID, "the context's tile order is for another frame");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = p->stream ? (hipStream_t)p->stream : ctx->stream;
    HIP_TRY(rtk::launch_assemble_tiles(slabs, frame, p->out_format == RT_OUT_F64, world, (long long)slab_elems,
                                       p->width, p->height, ctx->tile_order.as<uint32_t>(), s));
    return RT_OK;
}

int rt_tiles_assemble_host(const void* slabs, int64_t slab_elems, int world, int width, int height, int elem_bytes,
                           const uint32_t* order, void* frame)
{
    if (!slabs || !frame || world < 1 || width < 1 || height < 1 || (elem_bytes != 4 && elem_bytes != 8))
        return fail(RT_ERR_INVALID, "bad argument");
    const int tx = (width + 7) / 8;
    const int64_t n_tiles = (int64_t)tx * ((height + 7) / 8);
    const rtc::SlabLayout lay = rtc::slab_layout(width, height, 0, world, (size_t)elem_bytes);
    if (lay.n_max <= 0 || slab_elems < lay.slab_elems) return fail(RT_ERR_INVALID, "slab_elems below the largest shard's");
    if (order) {
        std::vector<uint8_t> seen((size_t)n_tiles, 0);
        for (int64_t i = 0; i < n_tiles; ++i) {
            if ((int64_t)order[i] >= n_tiles || seen[order[i]]) return fail(RT_ERR_INVALID, "order is not a permutation");
            seen[order[i]] = 1;
        }
    }
    const size_t px = 3 * (size_t)elem_bytes;
    const char* in = (const char*)slabs;
    char* out = (char*)frame;
    for (int r = 0; r < world; ++r) {
        const int n_r = rt_tiles_in_shard(width, height, r, world);
        for (int m = 0; m < n_r; ++m) {
            const int64_t pos = r + (int64_t)m * world;
            const int64_t t = order ? (int64_t)order[pos] : pos;
            const int x0 = (int)(t % tx) * 8, y0 = (int)(t / tx) * 8;
            for (int k = 0; k < 8 && y0 + k < height; ++k) {
                const int w = std::min(8, width - x0);
                std::memcpy(out + ((size_t)(y0 + k) * width + x0) * px,
                            in + ((size_t)r * slab_elems + ((size_t)k * 8 * n_r + 8 * (size_t)m) * 3) * elem_bytes,
                            (size_t)w * px);
            }
        }
    }
    return RT_OK;
}

int rt_cost_tile_order(const uint64_t* costs, int64_t n, uint32_t* order)
{
    if (n < 0 || (n > 0 && (!costs || !order)) || n > ((int64_t)1 << 32)) return fail(RT_ERR_INVALID, "bad argument");
    rtd::cost_order(costs, n, order);
    return RT_OK;
}

}  // extern "C"
