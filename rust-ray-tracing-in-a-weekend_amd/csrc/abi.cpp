// abi.cpp — the extern "C" boundary (include/rt/rt_abi.h). No exception and no
// C++ type crosses it; every entry point returns RT_OK or a negative RT_ERR_*.
// Here: the context (last error, build identity, create, destroy, upload, options, stats) and the
// render driver (run_range, rt_render, the accumulators). The entry points that touch no context
// are in abi_scene.cpp, the auxiliary passes in abi_passes.cpp, the post-filters in abi_filters.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rt/rt_abi.h"
#include "rt/rt_numerics.h"
#include "camera_rays.hpp"
#include "ctx_internal.hpp"
#include "deal_cache.hpp"
#include "launch_plan.hpp"
#include "primary_candidates.hpp"
#include "render_internal.hpp"
#include "scene_lower.hpp"
#include "trace_kernel.hpp"

namespace {

thread_local std::string g_last_error;

}  // namespace

int rtx::fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

int rtx::hip_fail(hipError_t e, const char* what)
{
    return fail(RT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The trace-output buffer's default bound: 64 GiB, or half the device's free memory if that is
// less (round 6). The per-sample buffer is as fast as the in-kernel ring reduction on the random
// scene and 1.4 % faster on the final scene, whose ring reductions stall a wave holding 4 waves'
// worth of path state per SIMD (interleaved medians, kernel + reduce ms: C2 74.47 vs 74.41, C2 f32
// 64.46 vs 64.38, C4 982.1 vs 996.2; profiles/r06c_ab_*.log), and a 288 GB device holds C4's
// 49.8 GB of records in one batch. The ring stays for renders the bound does not hold in one
// batch (C5: 1.6 TB of records), where its chunk partials are 1/16 of the bytes.
static size_t default_buf_cap()
{
    size_t fr = 0, tot = 0;
    size_t cap = (size_t)64 << 30;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr > 0) cap = std::min(cap, fr / 2);
    return std::max(cap >> 20, (size_t)1) << 20;
}

#ifndef RT_SRC_HASH
#define RT_SRC_HASH "unknown"
#endif

extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }
const char* rt_last_error(void) { return g_last_error.c_str(); }
const char* rt_build_info(void) { return RT_SRC_HASH; }

int rt_device_count(int* count)
{
    if (!count) return fail(RT_ERR_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return hip_fail(e, "hipGetDeviceCount");
    }
    *count = n;
    return RT_OK;
}

int rt_ctx_create(int device, rt_ctx** out)
{
    if (!out) return fail(RT_ERR_INVALID, "null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(RT_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    rt_ctx* c = new (std::nothrow) rt_ctx();
    if (!c) return fail(RT_ERR_OOM, "rt_ctx");
    c->device = device;
    c->sample_buf_cap = default_buf_cap();
    {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, device) == hipSuccess && v > 0)
            c->dev.lds_per_cu = (size_t)v;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && v > 0)
            c->dev.lds_per_block = (size_t)v;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0)
            c->dev.n_cus = v;
        c->dev.lds_per_block = std::min(c->dev.lds_per_block, c->dev.lds_per_cu);
    }
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&c->tstream[i], hipStreamNonBlocking);
    if (e == hipSuccess) e = c->ev.create();
    if (e == hipSuccess) e = c->flt_denoise.ev.create();
    if (e == hipSuccess) e = c->ev_ft.create();
    if (e == hipSuccess) e = c->ev_q.create();
    if (e == hipSuccess) e = c->flt_atrous.ev.create();
    if (e == hipSuccess) e = c->flt_cross.ev.create();
    if (e == hipSuccess) e = c->flt_pyramid.ev.create();
    if (e == hipSuccess) e = c->ev_pf.create(hipEventDisableTiming);
    if (e == hipSuccess) e = c->ev_done.create(hipEventDisableTiming);
    if (e == hipSuccess) e = c->ev_in.create(hipEventDisableTiming);
    if (e == hipSuccess) e = c->ev_tr.create(hipEventDisableTiming);
    if (e == hipSuccess) e = c->ev_rd.create(hipEventDisableTiming);
    if (e == hipSuccess) e = c->ev_pc.create();
    if (e == hipSuccess) e = c->counters.alloc(kCounters * sizeof(unsigned long long));
    if (e == hipSuccess) e = c->params.alloc(kParamSlots * sizeof(rtk::KParams));
    if (e == hipSuccess) e = c->work.alloc(2 * rtk::kDealTable * sizeof(unsigned));
    if (e != hipSuccess) {
        rt_ctx_destroy(c);   // (safe on a partly created context: null streams and events, empty buffers are skipped)
        return hip_fail(e, "rt_ctx_create");
    }
    *out = c;
    return RT_OK;
}

// Waits for everything the context enqueued, on its own streams and on a caller's; the buffers and
// events are members that free themselves.
void rt_ctx_destroy(rt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev_done.ev[0] && c->any_enqueued) (void)c->ev_done.wait(0);  // work on a caller's stream
    for (hipStream_t s : c->tstream) {
        if (s) (void)hipStreamSynchronize(s);
        if (s) (void)hipStreamDestroy(s);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// Everything the kernels assume about the scene is decided on the host by rtl::lower
// (scene_lower.cpp); this copies its tables and the SoA's others into one device allocation
// (256-B aligned tables) and records the rest in the context.
int rt_ctx_upload_soa(rt_ctx* c, const rt_scene_soa* s)
{
    if (!c || !s) return fail(RT_ERR_INVALID, "null argument");
    rtl::Lowered L;
    std::string err;
    const int rc = rtl::lower(*s, c->opt_hoist != 0, L, err);
    if (rc) return fail(rc, err);
    c->upload_gen++;   // the scene's tables are replaced below: a measured deal order is another scene's
    c->deal.drop();
    c->primary_valid = false;
    c->last_deal_n = 0;

    struct Table {
        const void* src;
        size_t bytes, off;
    } t[10] = {{L.nodes.data(), L.nodes.size() * sizeof(rt_bvh_node), 0},
               {s->prim_refs, (size_t)s->n_prim_refs * 4, 0},
               {L.prims.data(), L.prims.size() * sizeof(rt_prim), 0},
               {L.instances.data(), L.instances.size() * sizeof(rt_instance), 0},
               {s->materials, (size_t)s->n_materials * sizeof(rt_material), 0},
               {s->textures, (size_t)s->n_textures * sizeof(rt_texture), 0},
               {s->perlin_ranvec, (size_t)s->n_perlin * 768 * 8, 0},
               {s->perlin_perm, (size_t)s->n_perlin * 768 * 4, 0},
               {s->image_data, (size_t)s->image_bytes, 0},
               {L.leaf_prims.data(), L.leaf_prims.size() * sizeof(rt_prim), 0}};
    size_t total = 0;
    for (Table& e : t) {
        e.off = total;
        total = align_up(total + e.bytes, 256);
    }
    total = std::max<size_t>(total, 256);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->any_enqueued) HIP_TRY(c->ev_done.wait(0));  // renders still reading the scene
    const int rc_buf = c->scene_buf.reserve(c->stream, total);
    if (rc_buf) return rc_buf;
    char* base = c->scene_buf.as<char>();
    for (const Table& e : t)
        if (e.bytes) HIP_TRY(hipMemcpy(base + e.off, e.src, e.bytes, hipMemcpyHostToDevice));

    rtk::SceneDev& S = c->S;
    S.nodes = (const rt_bvh_node*)(base + t[0].off);
    S.prim_refs = (const int32_t*)(base + t[1].off);
    S.prims = (const rt_prim*)(base + t[2].off);
    S.instances = (const rt_instance*)(base + t[3].off);
    S.materials = (const rt_material*)(base + t[4].off);
    S.textures = (const rt_texture*)(base + t[5].off);
    S.perlin_ranvec = (const double*)(base + t[6].off);
    S.perlin_perm = (const int32_t*)(base + t[7].off);
    S.image = (const uint8_t*)(base + t[8].off);
    S.leaf_prims = (const rt_prim*)(base + t[9].off);
    S.tlas_root = s->tlas_root;
    S.pre_leaf = L.pre_leaf;
    S.pre_root = L.pre_root;
    std::copy(L.pre_lo, L.pre_lo + 3, S.pre_lo);
    std::copy(L.pre_hi, L.pre_hi + 3, S.pre_hi);
    S.stack16_ok = L.stack16_ok;
    S.blas_base = L.blas_base;
    S.stack_entries = L.stack_entries;
    S.n_tlas_nodes = L.n_tlas_nodes;
    S.n_blas_bfs = L.n_blas_bfs;
    S.n_lds_nodes = S.n_lds_blas = S.seed_stage_bytes = 0;   // a launch decides what it stages in LDS
    S.has_lights = L.has_lights;
    S.has_spheres = L.has_spheres;
    c->scene = rtp::scene_facts(L, *s);
    c->has_scene = true;
    c->stats.scene_bytes = (int64_t)total;
    return RT_OK;
}

int rt_ctx_upload_world(rt_ctx* c, rt_world* w, int accel)
{
    const rt_scene_soa* soa = nullptr;
    int rc = rt_world_flatten(w, accel, &soa);
    if (rc) return rc;
    return rt_ctx_upload_soa(c, soa);
}

// ---- render ----------------------------------------------------------------------------
// (the shard geometry itself: launch_plan.cpp)
int rt_rows_in_shard(int height, int row_begin, int row_stride) { return rtp::rows_in_shard(height, row_begin, row_stride); }
int rt_rows_in_band_shard(int height, int row_begin, int row_stride, int row_block)
{
    return rtp::rows_in_band_shard(height, row_begin, row_stride, row_block);
}
int rt_tiles_in_shard(int width, int height, int tile_begin, int tile_stride)
{
    return rtp::tiles_in_shard(width, height, tile_begin, tile_stride);
}

}  // extern "C"

// (documented in render_internal.hpp)
int fill_kparams(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const Layout& lay, int chunk,
                 const Sink& sink, int64_t img_tiles, rtk::KParams& K)
{
    std::memset(&K, 0, sizeof K);
    K.cam = *cam;
    for (int i = 0; i < 3; ++i) K.bg[i] = p->background[i];
    const rtc::CameraScales cs = rtc::camera_scales(*cam, p->width, p->height);   // (camera_rays.hpp: rt_camera_rays' too)
    K.scale_m11 = cs.scale_m11;
    K.scale_time = cs.scale_time;
    K.wm1 = cs.wm1;
    K.hm1 = cs.hm1;
    K.inv_wm1 = cs.inv_wm1;
    K.inv_hm1 = cs.inv_hm1;
    K.seed = p->render_seed;
    K.width = lay.w;
    K.height = p->height;
    K.img_width = p->width;
    K.max_depth = p->max_depth;
    K.spp_chunk = chunk;
    K.row_begin = p->row_begin;
    K.row_stride = p->row_stride;
    K.row_block_shift = 0;
    while ((1 << K.row_block_shift) < row_block_of(p)) K.row_block_shift++;
    K.tile_shard = p->tile_shard;
    K.img_tiles_x = (p->width + 7) / 8;
    {   // t / img_tiles_x by multiply-high: m = floor(2^32 / d) + 1 gives floor(t * m / 2^32) =
        // floor(t / d) whenever t * (m d - 2^32) < 2^32 (the excess stays under one step of t / d)
        const uint64_t d = (uint64_t)K.img_tiles_x, m = ((uint64_t)1 << 32) / std::max<uint64_t>(d, 1) + 1;
        const uint64_t e = m * d - ((uint64_t)1 << 32);
        K.tile_div_magic = (d >= 2 && m < ((uint64_t)1 << 32) && (uint64_t)img_tiles * e < ((uint64_t)1 << 32))
                               ? (uint32_t)m : 0u;
    }
    if (sink.moments) {   // the adaptive call's own order, dealt as a frame is (the order carries no cost ranking)
        K.tile_order = sink.moments->order;
    } else if (p->tile_shard && c->tile_order_n > 0) {   // the context's tile order: every tile shard takes it
        if (c->tile_order_n != img_tiles)
            return fail(RT_ERR_INVALID, "the tile order has " + std::to_string(c->tile_order_n) + " tiles, the frame " +
                                            std::to_string(img_tiles));
        K.tile_order = c->tile_order.as<uint32_t>();
        K.tile_major = 1;   // the order's first tiles done first and entirely (rt_abi.h rt_ctx_set_tile_order)
    }
    K.n_rows = lay.rows;
    K.tiles_x = (lay.w + 7) / 8;
    K.tiles_y = (lay.rows + 7) / 8;
    return RT_OK;
}

// The whole-frame deal order (deal_cache.hpp): what the cache decides for this render, carried out.
// The table and the tile costs follow each of the two work counters in memory (trace_kernel.hpp,
// kDealTable). A measuring render uploads the identity table, zeroes the costs and launches with
// tile_major = kDealMeasure; the next one of the key reads the costs back (the one synchronization,
// inside this call), builds the order and uploads it; later ones only set tile_major =
// kDealOrdered. `stream` already waits for the context's earlier work.
// RT_OPT_SKIP_SKY_TILES (sky_ok: this render may leave its all-sky tiles out, c->sky_flags): a render
// that goes through a table is dealt the table's unflagged tiles only — the identity table and the
// cost order alike, the cache's own order stays whole — and *dealt_tiles is how many that is. The
// device tables are written again whenever what they leave out (deal_sky_gen) is not what this
// render wants, so the option may change between two renders of a key.
static int deal_setup(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rtp::Plan& pl, bool adaptive_pass,
                      int64_t img_tiles, bool sky_ok, hipStream_t stream, rtk::KParams& K, int64_t* dealt_tiles)
{
    c->last_deal_n = 0;
    const bool ok = rtk::deal_variant(pl.variant) && rtd::eligible(*p, pl.schedule, adaptive_pass);
    const rtd::Decision d = c->deal.next(c->opt_deal, ok, rtd::key_of(c->upload_gen, *cam, *p), img_tiles);
    const size_t n = (size_t)img_tiles;
    const bool sky = sky_ok && (d.measure || d.ordered) && c->sky_flags.size() == n;
    const uint64_t want_gen = sky ? c->sky_gen : 0;
    // `order` (n raster tiles by position) without the tiles this render skips, to both tables
    const auto upload = [&](const uint32_t* order) -> hipError_t {
        std::vector<uint32_t> live;
        size_t m = n;
        if (sky) {
            live.reserve(n);
            for (size_t i = 0; i < n; ++i)
                if (!c->sky_flags[order[i]]) live.push_back(order[i]);
            order = live.data();
            m = live.size();
        }
        hipError_t e = hipSuccess;
        for (int h = 0; h < 2 && e == hipSuccess; ++h)
            e = hipMemcpyAsync(c->work.as<unsigned>() + h * c->work_stride + rtk::kDealTable, order, m * sizeof(uint32_t),
                               hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);   // (the source is pageable, and local when filtered)
        if (e == hipSuccess) c->deal_sky_gen = want_gen;
        return e;
    };
    if (d.measure) {
        if (img_tiles > c->deal_cap) {   // (a key's first render: no work on the context's streams reads them)
            HIP_TRY(hipStreamSynchronize(stream));
            const size_t stride = rtk::kDealTable + 2 * n;
            DevBuf w;   // the new block first: the old one is freed only once this succeeded, so c->work stays valid
            const hipError_t e = w.alloc(2 * stride * sizeof(unsigned));
            if (e != hipSuccess) {
                c->deal.drop();
                return hip_fail(e, "deal order table");
            }
            c->work = std::move(w);
            c->work_stride = stride;
            c->deal_cap = img_tiles;
        }
        std::vector<uint32_t> raster(n);
        for (size_t i = 0; i < n; ++i) raster[i] = (uint32_t)i;
        for (int h = 0; h < 2; ++h)
            HIP_TRY(hipMemsetAsync(c->work.as<unsigned>() + h * c->work_stride + rtk::kDealTable + n, 0, n * sizeof(unsigned), stream));
        HIP_TRY(upload(raster.data()));
        K.tile_major = rtk::kDealMeasure;
    }
    if (d.build) {
        std::vector<uint32_t> part(2 * n);
        hipError_t e = hipSuccess;
        for (int h = 0; h < 2 && e == hipSuccess; ++h)
            e = hipMemcpyAsync(part.data() + h * n, c->work.as<unsigned>() + h * c->work_stride + rtk::kDealTable + n, n * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            c->deal.fail_build();
            return hip_fail(e, "deal order: tile costs");
        }
        std::vector<uint64_t> costs(n);   // (overlapped batches count on both counters' tables)
        for (size_t i = 0; i < n; ++i) costs[i] = (uint64_t)part[i] + part[n + i];
        e = upload(c->deal.finish_build(costs.data()).data());   // (a tile the measuring render skipped: cost 0, at the end)
        if (e != hipSuccess) {
            c->deal.fail_build();
            return hip_fail(e, "deal order: upload");
        }
    } else if (d.ordered && c->deal_sky_gen != want_gen) {
        const hipError_t e = upload(c->deal.order().data());
        if (e != hipSuccess) {
            c->deal.drop();
            return hip_fail(e, "deal order: upload");
        }
    }
    if (d.ordered) {
        K.tile_major = rtk::kDealOrdered;
        c->last_deal_n = img_tiles;
    }
    if (sky) {
        *dealt_tiles = img_tiles - c->sky_n;
        c->stats.sky_tiles = c->sky_n;
    }
    return RT_OK;
}

// RT_OPT_PRIMARY_CANDIDATES: the candidate table of this render's (scene upload, camera, frame size),
// built here when the key (or the forced k) changed — the cost real use pays, once per key; the one
// synchronization reads its build time and flagged count — and handed to the launch. Only the f64
// spheres variant's timed staged per-sample pool kernels read it (trace_launch.hpp picks the
// CfgPrimary instantiation); any other render, or a frame whose table would exceed
// rtpc::kMaxTableBytes, walks every primary ray. `stream` already waits for the context's earlier work.
// The table's all-sky tile flags (RT_OPT_SKIP_SKY_TILES) are built, kept and replaced with it.
static int primary_setup(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rtp::Plan& pl, bool count_work,
                         hipStream_t stream, rtk::KParams& K, rtk::LaunchOpts& o)
{
    rt_stats& st = c->stats;
    st.primary_table_bytes = 0;
    st.primary_build_ms = 0.0;
    st.primary_walk_share = 0.0;
    st.defer_roots = 0;
    const size_t bytes = rtpc::table_bytes(p->width, p->height);
    if (!c->opt_primary || pl.variant != rtk::FEAT_SET_SPHERES || pl.f32 || pl.schedule != RT_SCHED_POOL || !pl.shape.s16 ||
        pl.seed_stage_bytes == 0 || count_work || bytes > rtpc::kMaxTableBytes || p->width < 2 || p->height < 2)
        return RT_OK;
    rtd::Key key = rtd::key_of(c->upload_gen, *cam, *p);
    key.row_begin = 0;
    key.row_stride = key.row_block = 1;
    if (!(c->primary_valid && rtd::same_key(key, c->primary_key) && c->primary_k == c->opt_primary_k)) {
        c->primary_valid = false;
        int rc = c->primary_tab.reserve(stream, bytes + 16);
        if (rc) return rc;
        const size_t n_tiles = (size_t)rtpc::tiles_x_of(p->width) * (size_t)rtpc::tiles_y_of(p->height);
        rc = c->sky_tab.reserve(stream, 16 + n_tiles);
        if (rc) return rc;
        unsigned* const flagged = reinterpret_cast<unsigned*>(c->primary_tab.as<char>() + bytes);
        HIP_TRY(c->ev_pc.record(0, stream));
        HIP_TRY(rtk::launch_primary_candidates(c->S, *cam, p->width, p->height, c->opt_primary_k, c->primary_tab.p, flagged, stream));
        // its all-sky tiles (RT_OPT_SKIP_SKY_TILES), whatever the option says now: it may change while the table is kept
        HIP_TRY(rtk::launch_primary_sky_tiles(c->primary_tab.p, p->width, p->height, c->sky_dev(), c->sky_tab.as<unsigned>(), stream));
        HIP_TRY(c->ev_pc.record(1, stream));
        unsigned n_flagged = 0, n_sky = 0;
        c->sky_flags.assign(n_tiles, 0);
        HIP_TRY(hipMemcpyAsync(&n_flagged, flagged, sizeof n_flagged, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&n_sky, c->sky_tab.p, sizeof n_sky, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(c->sky_flags.data(), c->sky_dev(), n_tiles, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        c->sky_n = (int64_t)n_sky;
        c->sky_gen++;
        float ms = 0.0f;
        HIP_TRY(c->ev_pc.elapsed(0, &ms));
        c->primary_key = key;
        c->primary_k = c->opt_primary_k;
        c->primary_flagged = (int64_t)n_flagged;
        c->primary_valid = true;
        st.primary_build_ms = ms;
    }
    K.primary = c->primary_tab.as<uint4>();
    o.primary = 1;
    o.defer_roots = c->opt_defer_roots;   // the CfgDefer kernel, which exists wherever the primary-candidate one does
    st.defer_roots = c->opt_defer_roots;
    st.primary_table_bytes = (int64_t)bytes;
    st.primary_walk_share = (double)c->primary_flagged / ((double)p->width * (double)p->height);
    return RT_OK;
}

// What rt_last_stats shows of a planned range (an empty range: the all-zero plan); the timings,
// the counters and waves_per_simd are filled when the events resolve.
static void write_stats(rt_ctx* c, const rtp::Plan& pl, int chunk, int waves_per_simd, bool count)
{
    rt_stats& st = c->stats;
    st.lds_nodes = pl.n_lds_nodes;
    st.variant_features = (int32_t)pl.variant;
    st.slab32 = pl.slab32;
    st.lds_stack = pl.lds_stack;
    st.schedule = pl.schedule;
    st.precision = pl.f32 ? RT_PREC_F32 : RT_PREC_F64;
    st.waves_per_simd = waves_per_simd;
    st.n_batches = pl.n_batches;
    st.ring_bytes = (int64_t)pl.ring_bytes;
    st.trace_buf_bytes = (int64_t)pl.trace_buf_bytes;
    st.overlapped = pl.overlap ? 1 : 0;
    st.n_chunks = pl.n_chunks;
    st.samples = (uint64_t)pl.px * (uint64_t)pl.total;   // (the all-zero plan: px 1, no samples)
    st.n_items = (uint64_t)pl.px * (uint64_t)pl.n_chunks;
    st.spp_chunk = chunk;
    st.node_bytes = (int32_t)sizeof(rt_bvh_node);
    st.prim_bytes = (int32_t)sizeof(rt_prim);
    st.material_bytes = (int32_t)sizeof(rt_material);
    c->ev.arm();
    c->pending_counts = count;
    if (!st.samples) st.casts = st.node_visits = st.prim_tests = 0;
}

// Traces samples [s_begin, s_end) of the shard in chunks of `chunk` and reduces them into
// the sink, as rtp::plan (launch_plan.cpp) lays the range out. Events: ev[0] before the first
// trace launch, ev[1] after the last one, ev[2] after the last reduction. Chunk and item
// schedules: chunk partials per launch, reduced in chunk order (or added to the sink's / a
// running accumulator across buffer batches). Per-sample pool: per-sample radiance in batches;
// with more than one batch (or an acc sink) the sums run through an accumulator plus the open
// chunk's sum (carried across batches), which keeps the additions in the one-batch order.
int run_range(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int s_begin, int s_end, int chunk,
              hipStream_t stream, const Sink& sink)
{
    const Layout lay = layout_of(p);
    const long long n_px = (long long)lay.rows * lay.w;
    if (n_px == 0 || s_end <= s_begin) {
        // an empty shard (rt_rows_in_shard / rt_tiles_in_shard 0: a rank past the tile count)
        // or an empty sample range: nothing to trace or write; the events still bracket the
        // (empty) work so rt_last_stats resolves
        for (int i = 0; i < 3; ++i) HIP_TRY(c->ev.record(i, stream));
        write_stats(c, rtp::Plan{}, chunk, 0, false);
        c->last_deal_n = 0;
        c->stats.sky_tiles = 0;
        return RT_OK;
    }

    const int64_t img_tiles = (int64_t)((p->width + 7) / 8) * ((p->height + 7) / 8);
    rtk::KParams K;
    int rc = fill_kparams(c, cam, p, lay, chunk, sink, img_tiles, K);
    if (rc) return rc;

    rtp::Request rq;
    rq.lay = lay;
    rq.s_begin = s_begin;
    rq.s_end = s_end;
    rq.chunk = chunk;
    rq.count_work = p->count_work != 0;
    rq.acc_sink = sink.acc != nullptr;
    rq.moments = sink.moments != nullptr;
    rq.cam_mag = rtp::camera_magnitude(*cam);
    rq.cam_time0 = cam->time0;
    rq.cam_time1 = cam->time1;
    // the plan, and its buffers: an attempt whose trace output (or ring) does not fit the device
    // is planned again without the ring, or under half the bound (this render only: the
    // context's bound stays, so a later render on it uses the memory freed since)
    rtp::Retry retry{c->sample_buf_cap, true};
    rtp::Plan pl;
    for (;;) {
        pl = rtp::plan(c->scene, c->dev, c->opt, rq, retry);
        if (pl.err) return fail(pl.err, pl.err_msg);
        rc = c->acc_tmp.reserve(stream, pl.acc_bytes);
        if (rc) return rc;
        bool oom = false;
        rc = c->partial.reserve(stream, pl.partial_bytes, &oom);
        if (rc == RT_OK && pl.ring) {
            rc = c->ring.reserve(stream, pl.ring_bytes, &oom);
            if (rc != RT_OK && oom) {   // no room for the ring: the per-sample buffer, as before
                retry.ring_allowed = false;
                continue;
            }
        }
        if (rc == RT_OK) break;
        if (!oom) return rc;
        if (!rtp::shrink(pl, retry)) return hip_fail(hipErrorOutOfMemory, "trace output buffer (smallest batch)");
    }
    // acc_tmp = [open chunk sums | running total (no acc sink)], or the running total alone
    double* const acc_tmp = c->acc_tmp.as<double>();
    double* const open = pl.open_chunk ? acc_tmp : nullptr;
    double* const acc = !pl.own_total ? sink.acc : pl.open_chunk ? acc_tmp + pl.px * 3 : acc_tmp;
    PlannedLaunch launch = planned_launch(c->S, pl);
    const rtk::SceneDev& S = launch.S;
    K.block_chunks = pl.block_chunks;
    K.block_samples = pl.block_samples;
    K.ring_waves = pl.ring_waves;
    int waves_per_simd = 0;
    rtk::LaunchOpts& o = launch.o;
    o.count = rq.count_work;
    o.waves_per_simd = &waves_per_simd;
    const rtk::SampleTiles tiles{lay.w, lay.rows, (lay.w + 7) / 8, pl.f32};
    rc = primary_setup(c, cam, p, pl, rq.count_work, stream, K, o);
    if (rc) return rc;
    // RT_OPT_SKIP_SKY_TILES: a direct render with a table, through the per-sample buffer in one batch
    // (reduce_samples_tiled takes the flags; the carry form and the ring's chunk partials do not, so
    // those renders trace every tile), at max_depth >= 1 (at 0 every sample is black, not the
    // background). deal_setup adds its own condition: the render goes through a deal table.
    const bool sky_ok = c->opt_sky && o.primary && p->max_depth >= 1 && !sink.acc && !sink.moments && pl.per_sample &&
                        !pl.ring && pl.n_batches == 1 && !open && c->sky_n > 0 && c->sky_n < img_tiles;
    int64_t dealt_tiles = (int64_t)K.tiles_x * K.tiles_y;
    c->stats.sky_tiles = 0;
    rc = deal_setup(c, cam, p, pl, sink.moments != nullptr, img_tiles, sky_ok, stream, K, &dealt_tiles);
    if (rc) return rc;
    rtk::SkyTiles sky;
    if (c->stats.sky_tiles > 0) {
        sky.flags = c->sky_dev();
        for (int i = 0; i < 3; ++i) sky.rec[i] = 0.0 + 1.0 * K.bg[i];   // a sample that meets nothing: cr = 0 + T * bg, T = 1
    }

    if (pl.own_total) HIP_TRY(hipMemsetAsync(acc, 0, pl.px_bytes, stream));
    if (rq.count_work) {
        HIP_TRY(hipMemsetAsync(c->counters.p, 0, kCounters * sizeof(unsigned long long), stream));
        rc = c->tile_cost.reserve(stream, (size_t)img_tiles * sizeof(unsigned long long));
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(c->tile_cost.p, 0, (size_t)img_tiles * sizeof(unsigned long long), stream));
        K.tile_cost = c->tile_cost.as<unsigned long long>();
        // (the pool kernels count them; the chunk schedule does not)
        c->tile_cost_n = pl.schedule == RT_SCHED_POOL || pl.schedule == RT_SCHED_ITEMS ? img_tiles : 0;
    }
    HIP_TRY(c->ev.record(0, stream));
    // overlapped batches: both trace streams start after everything enqueued on `stream` so far
    if (pl.overlap) {
        HIP_TRY(c->ev_in.record(0, stream));
        for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamWaitEvent(c->tstream[i], c->ev_in.ev[0], 0));
    }
    for (int bi = 0; bi < pl.n_batches; ++bi) {
        const int b0 = s_begin + (int)(bi * pl.batch);
        const int b1 = (int)std::min<long long>(s_end, b0 + pl.batch);
        K.sample_begin = b0;
        K.spp = b1;
        K.n_chunks = (b1 - b0 + chunk - 1) / chunk;
        {
            const bool items = pl.schedule == RT_SCHED_ITEMS;
            const unsigned g = items ? (unsigned)K.block_chunks : (unsigned)K.block_samples;   // (POOL: samples)
            const unsigned n = items ? (unsigned)K.n_chunks : (unsigned)(K.spp - K.sample_begin);
            const unsigned n_groups = (n + g - 1) / std::max(g, 1u);
            K.n_work_blocks = (unsigned)dealt_tiles * n_groups;
            K.deal_div = K.tile_major ? n_groups : (unsigned)K.tiles_x * (unsigned)K.tiles_y;
        }
        // batch bi's buffer half, trace stream and work counter (one of each per overlapped batch)
        const int h = pl.overlap ? (bi & 1) : 0;
        double* buf = c->partial.as<double>() + (size_t)h * (pl.half_bytes / sizeof(double));
        hipStream_t ts = pl.overlap ? c->tstream[h] : stream;
        K.ring = pl.ring ? c->ring.as<double>() + (size_t)h * (pl.ring_one_bytes / sizeof(double)) : nullptr;   // one ring per trace stream
        if (pl.overlap && bi >= 2) HIP_TRY(hipStreamWaitEvent(ts, c->ev_rd.ev[h], 0));   // batch bi - 2 reduced: half free
        rtk::KParams* dK = c->params.as<rtk::KParams>() + c->param_slot;
        c->param_slot = (c->param_slot + 1) % kParamSlots;
        HIP_TRY(hipMemcpyAsync(dK, &K, sizeof K, hipMemcpyHostToDevice, ts));
        HIP_TRY(rtk::launch_trace(S, K, dK, buf, c->counters.as<unsigned long long>(),
                                  c->work.as<unsigned>() + h * c->work_stride, o, ts));
        if (bi == pl.n_batches - 1) HIP_TRY(c->ev.record(1, ts));
        if (pl.overlap) {   // reduce in batch order on `stream`, after this batch's trace
            HIP_TRY(c->ev_tr.record(h, ts));
            HIP_TRY(hipStreamWaitEvent(stream, c->ev_tr.ev[h], 0));
        }
        if (sink.moments) {
            HIP_TRY(rtk::launch_adaptive_moments(buf, *sink.moments, K.tiles_x, b1 - b0, chunk,
                                                 (int)(((long long)b0 - s_begin) % chunk), bi == pl.n_batches - 1,
                                                 sink.n_done, stream, sink.halves, b0));
        } else if (!pl.per_sample) {
            if (acc) HIP_TRY(rtk::launch_accumulate(buf, acc, n_px, K.n_chunks, stream));
            else HIP_TRY(rtk::launch_reduce(buf, sink.out, sink.f64, n_px, K.n_chunks, sink.scale, stream));
        } else if (!open) {
            HIP_TRY(rtk::launch_reduce_samples(buf, sink.out, sink.f64, tiles, b1 - b0, chunk, sink.scale, stream, sky));
        } else {
            HIP_TRY(rtk::launch_reduce_samples_carry(buf, acc, open, tiles, b1 - b0, chunk,
                                                     (int)(((long long)b0 - s_begin) % chunk), bi == pl.n_batches - 1,
                                                     stream));
        }
        if (pl.overlap) HIP_TRY(c->ev_rd.record(h, stream));
    }
    if (pl.own_total)  // resolve the running sums: 0.0 + sum, times scale, as one batch does
        HIP_TRY(rtk::launch_reduce(acc, sink.out, sink.f64, n_px, 1, sink.scale, stream));
    HIP_TRY(c->ev.record(2, stream));
    write_stats(c, pl, chunk, waves_per_simd, rq.count_work);
    return RT_OK;
}

extern "C" {

int rt_render(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, void* out)
{
    if (!c || !cam || !p || !out) return fail(RT_ERR_INVALID, "null argument");
    if (!c->has_scene) return fail(RT_ERR_NO_SCENE, "no scene uploaded");
    if (bad_geometry(p) || p->spp < 1 || p->max_depth < 0 || (p->out_format != RT_OUT_F32 && p->out_format != RT_OUT_F64))
        return fail(RT_ERR_INVALID, "bad render params");
    const Layout lay = layout_of(p);
    const int chunk = p->spp_chunk > 0 ? std::min(p->spp_chunk, p->spp) : auto_chunk(p->spp);
    const long long n_px = (long long)lay.rows * lay.w;

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;
    const size_t out_bytes = (size_t)n_px * 3 * (p->out_format == RT_OUT_F64 ? 8 : 4);
    void* dev_out = out;
    if (!p->out_on_device) {
        rc = c->out_buf.reserve(stream, std::max<size_t>(out_bytes, 16));
        if (rc) return rc;
        dev_out = c->out_buf.p;
    }
    Sink sink;
    sink.out = dev_out;
    sink.f64 = p->out_format == RT_OUT_F64;
    sink.scale = 1.0 / (double)p->spp;
    rc = run_range(c, cam, p, 0, p->spp, chunk, stream, sink);
    if (rc) return rc;
    if (!p->out_on_device) HIP_TRY(hipMemcpyAsync(out, dev_out, out_bytes, hipMemcpyDeviceToHost, stream));
    rc = scope.end();
    if (rc) return rc;
    if (!p->out_on_device) HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

// ---- progressive accumulation -----------------------------------------------------------------
struct rt_accum {
    rt_ctx* ctx = nullptr;
    int width = 0, height = 0, row_begin = 0, row_stride = 1, row_block = 1, tile_shard = 0, n_rows = 0, chunk = 1;
    long long n_px = 0;
    int64_t done = 0;
    DevBuf sums;                        // device, n_px x 3 f64
    hipStream_t last_stream = nullptr;  // the stream the last batch was enqueued on
};

int rt_accum_create(rt_ctx* c, const rt_render_params* p, rt_accum** out)
{
    if (!c || !p || !out) return fail(RT_ERR_INVALID, "null argument");
    *out = nullptr;
    if (bad_geometry(p) || p->spp < 0 || (p->spp_chunk == 0 && p->spp < 1))
        return fail(RT_ERR_INVALID, "bad accumulator geometry");
    auto* a = new (std::nothrow) rt_accum;
    if (!a) return fail(RT_ERR_OOM, "out of host memory");
    a->ctx = c;
    a->width = p->width;
    a->height = p->height;
    a->row_begin = p->row_begin;
    a->row_stride = p->row_stride;
    a->row_block = row_block_of(p);
    a->tile_shard = p->tile_shard;
    const Layout lay = layout_of(p);
    a->n_rows = lay.rows;
    a->chunk = p->spp_chunk > 0 ? p->spp_chunk : auto_chunk(p->spp);
    a->n_px = (long long)lay.rows * lay.w;
    a->last_stream = c->stream;
    const size_t bytes = (size_t)std::max<long long>(a->n_px, 1) * 3 * sizeof(double);
    hipError_t e = hipSetDevice(c->device);
    if (e == hipSuccess) e = a->sums.alloc(bytes);
    if (e == hipSuccess) e = hipMemset(a->sums.p, 0, bytes);
    if (e != hipSuccess) {
        delete a;
        return hip_fail(e, "rt_accum_create");
    }
    *out = a;
    return RT_OK;
}

void rt_accum_destroy(rt_accum* a)
{
    if (!a) return;
    (void)hipSetDevice(a->ctx->device);
    (void)hipStreamSynchronize(a->last_stream);
    delete a;
}

int rt_accum_add(rt_ctx* c, rt_accum* a, const rt_camera* cam, const rt_render_params* p, int sample_count)
{
    if (!c || !a || !cam || !p) return fail(RT_ERR_INVALID, "null argument");
    if (a->ctx != c) return fail(RT_ERR_INVALID, "accumulator belongs to another context");
    if (!c->has_scene) return fail(RT_ERR_NO_SCENE, "no scene uploaded");
    if (p->width != a->width || p->height != a->height || p->row_begin != a->row_begin ||
        p->row_stride != a->row_stride || row_block_of(p) != a->row_block || p->tile_shard != a->tile_shard)
        return fail(RT_ERR_INVALID, "render params do not match the accumulator's shard");
    if (sample_count < 0 || p->max_depth < 0 || a->done + sample_count > 0x7fffffffLL)
        return fail(RT_ERR_INVALID, "bad sample range");
    if (sample_count == 0) return RT_OK;
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    if (stream != a->last_stream) HIP_TRY(hipStreamSynchronize(a->last_stream));
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;
    a->last_stream = stream;   // the sums' stream from here on, even if a launch below fails
    Sink sink;
    sink.acc = a->sums.as<double>();
    rc = run_range(c, cam, p, (int)a->done, (int)(a->done + sample_count), a->chunk, stream, sink);
    if (rc) return rc;
    rc = scope.end();
    if (rc) return rc;
    a->done += sample_count;
    return RT_OK;
}

int rt_accum_get(rt_accum* a, double* sums, int64_t* samples_done)
{
    if (!a) return fail(RT_ERR_INVALID, "null argument");
    if (samples_done) *samples_done = a->done;
    if (!sums) return RT_OK;
    HIP_TRY(hipSetDevice(a->ctx->device));
    HIP_TRY(hipStreamSynchronize(a->last_stream));
    HIP_TRY(hipMemcpy(sums, a->sums.p, (size_t)a->n_px * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_accum_set(rt_accum* a, const double* sums, int64_t samples_done)
{
    if (!a || !sums) return fail(RT_ERR_INVALID, "null argument");
    if (samples_done < 0 || samples_done > 0x7fffffffLL) return fail(RT_ERR_INVALID, "bad sample count");
    HIP_TRY(hipSetDevice(a->ctx->device));
    HIP_TRY(hipStreamSynchronize(a->last_stream));
    HIP_TRY(hipMemcpy(a->sums.p, sums, (size_t)a->n_px * 3 * sizeof(double), hipMemcpyHostToDevice));
    a->done = samples_done;
    return RT_OK;
}

int rt_accum_resolve(rt_ctx* c, rt_accum* a, double divisor, int out_format, int out_on_device, void* out)
{
    if (!c || !a || !out) return fail(RT_ERR_INVALID, "null argument");
    if (a->ctx != c) return fail(RT_ERR_INVALID, "accumulator belongs to another context");
    if (out_format != RT_OUT_F32 && out_format != RT_OUT_F64) return fail(RT_ERR_INVALID, "bad output format");
    if (divisor == 0.0) divisor = (double)a->done;
    if (!(divisor > 0.0) || !std::isfinite(divisor)) return fail(RT_ERR_INVALID, "nothing accumulated / bad divisor");
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = a->last_stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;
    const size_t out_bytes = (size_t)a->n_px * 3 * (out_format == RT_OUT_F64 ? 8 : 4);
    void* dev_out = out;
    if (!out_on_device) {
        rc = c->out_buf.reserve(stream, std::max<size_t>(out_bytes, 16));
        if (rc) return rc;
        dev_out = c->out_buf.p;
    }
    // one "chunk" holding the running sums: 0.0 + sum = sum, then * (1/divisor) as rt_render
    HIP_TRY(rtk::launch_reduce(a->sums.as<double>(), dev_out, out_format == RT_OUT_F64, a->n_px, 1, 1.0 / divisor, stream));
    if (!out_on_device) HIP_TRY(hipMemcpyAsync(out, dev_out, out_bytes, hipMemcpyDeviceToHost, stream));
    rc = scope.end();
    if (rc) return rc;
    if (!out_on_device) HIP_TRY(hipStreamSynchronize(stream));
    return RT_OK;
}

int rt_render_progressive(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int batch_spp,
                          rt_progress_fn progress, void* user, void* out)
{
    if (!c || !cam || !p || !out) return fail(RT_ERR_INVALID, "null argument");
    if (p->spp < 1 || batch_spp < 1) return fail(RT_ERR_INVALID, "bad spp / batch");
    rt_accum* a = nullptr;
    int rc = rt_accum_create(c, p, &a);
    if (rc) return rc;
    const int batch = (batch_spp + a->chunk - 1) / a->chunk * a->chunk;  // keep chunk boundaries
    while (rc == RT_OK && a->done < p->spp) {
        const int n = (int)std::min<int64_t>(batch, p->spp - a->done);
        rc = rt_accum_add(c, a, cam, p, n);
        if (rc) break;
        if (progress) {
            hipError_t e = hipStreamSynchronize(a->last_stream);
            if (e != hipSuccess) {
                rc = hip_fail(e, "rt_render_progressive");
                break;
            }
            if (progress(user, a->done, p->spp)) break;
        }
    }
    if (rc == RT_OK)
        rc = rt_accum_resolve(c, a, a->done == p->spp ? (double)p->spp : 0.0, p->out_format, p->out_on_device, out);
    if (rc == RT_OK && p->out_on_device) {
        hipError_t e = hipStreamSynchronize(a->last_stream);  // the accumulator is freed below
        if (e != hipSuccess) rc = hip_fail(e, "rt_render_progressive");
    }
    rt_accum_destroy(a);
    return rc;
}

int rt_last_stats(rt_ctx* c, rt_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    if (c->ev.pending) {
        HIP_TRY(hipSetDevice(c->device));
        float ms[2] = {0, 0};
        const int rc = c->ev.resolve(ms);
        if (rc) return rc;
        c->stats.kernel_ms = ms[0];
        c->stats.reduce_ms = ms[1];
        unsigned long long (&h)[kCounters] = c->raw_counters;   // (zeros when the render counted no work)
        std::memset(h, 0, sizeof h);
        if (c->pending_counts) HIP_TRY(hipMemcpy(h, c->counters.p, sizeof h, hipMemcpyDeviceToHost));
        c->stats.casts = h[rtk::kCtrCasts];
        c->stats.node_visits = h[rtk::kCtrNodeVisits];
        c->stats.prim_tests = h[rtk::kCtrPrimTests];
        c->stats.cycles_camera = h[rtk::kCtrCyclesCamera];
        c->stats.cycles_trace = h[rtk::kCtrCyclesTrace];
        c->stats.cycles_shade = h[rtk::kCtrCyclesShade];
        c->stats.wave_steps = h[rtk::kCtrWaveSteps];
        c->stats.wave_node_steps = h[rtk::kCtrWaveNodeSteps];
        c->stats.cycles_nodes = h[rtk::kCtrCyclesNodes];
        c->stats.cycles_leaves = h[rtk::kCtrCyclesLeaves];
        c->stats.wave_leaf_steps = h[rtk::kCtrWaveLeafSteps];
        c->stats.camera_lanes = h[rtk::kCtrCameraLanes];
        c->stats.camera_steps = h[rtk::kCtrCameraSteps];
        c->stats.shade_lanes = h[rtk::kCtrShadeLanes];
        c->stats.shade_steps = h[rtk::kCtrShadeSteps];
    }
    *out = c->stats;
    return RT_OK;
}

int rt_last_tile_costs(rt_ctx* c, uint64_t* out, int64_t n)
{
    if (!c || (!out && n > 0) || n < 0) return fail(RT_ERR_INVALID, "bad argument");
    rt_stats st;
    const int rc = rt_last_stats(c, &st);   // the last render done
    if (rc) return rc;
    if (!c->pending_counts || c->tile_cost_n == 0) return 0;   // the last render counted no tile costs
    const int64_t m = std::min<int64_t>(n, c->tile_cost_n);
    if (m > 0) HIP_TRY(hipMemcpy(out, c->tile_cost.p, (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return (int)c->tile_cost_n;
}

int rt_ctx_set_tile_order(rt_ctx* c, const uint32_t* order, int64_t n)
{
    if (!c || n < 0 || (n > 0 && !order)) return fail(RT_ERR_INVALID, "bad argument");
    if (n > ((int64_t)1 << 30)) return fail(RT_ERR_INVALID, "tile order too long");
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        if ((int64_t)order[i] >= n || seen[order[i]]) return fail(RT_ERR_INVALID, "the tile order is not a permutation of 0..n-1");
        seen[order[i]] = 1;
    }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());   // no render still reads the old order
    c->tile_order.release();
    c->tile_order_n = 0;
    if (n == 0) return RT_OK;
    HIP_TRY(c->tile_order.alloc((size_t)n * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(c->tile_order.p, order, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->tile_order_n = n;
    return RT_OK;
}

int rt_last_deal_order(rt_ctx* c, uint32_t* out, int64_t n)
{
    if (!c || (!out && n > 0) || n < 0) return fail(RT_ERR_INVALID, "bad argument");
    if (c->last_deal_n == 0) return 0;   // the last render was dealt in raster order
    const std::vector<uint32_t>& order = c->deal.order();
    const int64_t m = std::min<int64_t>(n, (int64_t)order.size());
    if (m > 0) std::memcpy(out, order.data(), (size_t)m * sizeof(uint32_t));
    return (int)c->last_deal_n;
}

int rt_last_counters(rt_ctx* c, uint64_t* out, int n)
{
    if (!c || !out || n < 0) return fail(RT_ERR_INVALID, "null argument");
    rt_stats st;
    const int rc = rt_last_stats(c, &st);   // resolves a pending render's counters
    if (rc) return rc;
    for (int i = 0; i < n; ++i) out[i] = i < kCounters ? (uint64_t)c->raw_counters[i] : 0;
    return std::min(n, kCounters);
}

// ---- options and self test ----------------------------------------------------------------------
int rt_ctx_set_variant(rt_ctx* c, int slab32, int lds_stack, int lds_nodes)
{
    if (!c || slab32 < 0 || slab32 > 1 || lds_stack < 0 || lds_stack > 1 || lds_nodes < 0 || lds_nodes > 1)
        return fail(RT_ERR_INVALID, "bad variant");
    c->opt.slab32 = slab32;
    c->opt.lds_stack = lds_stack;
    c->opt.lds_nodes = lds_nodes;
    return RT_OK;
}

int rt_ctx_set_precision(rt_ctx* c, int precision)
{
    if (!c || (precision != RT_PREC_F64 && precision != RT_PREC_F32)) return fail(RT_ERR_INVALID, "bad precision");
    c->opt.precision = precision;
    return RT_OK;
}

int rt_ctx_set_option(rt_ctx* c, int key, int64_t v)
{
    if (!c) return fail(RT_ERR_INVALID, "null context");
    switch (key) {
    case RT_OPT_TRACE_BUF_BYTES:
        if (v < 0) return fail(RT_ERR_INVALID, "negative buffer bound");
        c->sample_buf_cap = v == 0 ? default_buf_cap() : std::max<size_t>((size_t)v, (size_t)1 << 20);
        return RT_OK;
    case RT_OPT_BATCH_OVERLAP: c->opt.overlap = v != 0; return RT_OK;
    case RT_OPT_BLOCK_SAMPLES:
        if (v < 0 || v > 1024) return fail(RT_ERR_INVALID, "block samples out of range (0..1024)");
        c->opt.block_samples = (int)v;
        return RT_OK;
    case RT_OPT_BLOCK_CHUNKS:
        if (v < 0 || v > 64) return fail(RT_ERR_INVALID, "block chunks out of range (0..64)");
        c->opt.block_chunks = (int)v;
        return RT_OK;
    case RT_OPT_EXTRA_FEATURES:
        if (v < 0 || (v & ~(int64_t)rtk::FEAT_ALL)) return fail(RT_ERR_INVALID, "unknown feature bits");
        c->opt.extra_features = (uint32_t)v;
        return RT_OK;
    case RT_OPT_HOIST: c->opt_hoist = v != 0; return RT_OK;
    case RT_OPT_POOL_RING:
        if (v < 0 || v > 2) return fail(RT_ERR_INVALID, "pool ring mode out of range (0 never, 1 when needed, 2 always)");
        c->opt.ring = (int)v;
        return RT_OK;
    case RT_OPT_COMM_DIRECT: c->opt_comm_direct = v != 0; return RT_OK;
    case RT_OPT_AUTO_DEAL_ORDER:
        if (v < 0 || v > 2) return fail(RT_ERR_INVALID, "deal order mode out of range (0 off, 1 auto, 2 measure only)");
        c->opt_deal = (int)v;
        return RT_OK;
    case RT_OPT_PRIMARY_CANDIDATES:
        if (v < 0 || v > 1) return fail(RT_ERR_INVALID, "primary candidates out of range (0 off, 1 on)");
        c->opt_primary = (int)v;
        return RT_OK;
    case RT_OPT_PRIMARY_CANDIDATES_K:
        if (v < 1 || v > rtpc::kSlots) return fail(RT_ERR_INVALID, "primary candidates per pixel out of range (1..7)");
        c->opt_primary_k = (int)v;
        return RT_OK;
    case RT_OPT_SKIP_SKY_TILES:
        if (v < 0 || v > 1) return fail(RT_ERR_INVALID, "skip sky tiles out of range (0 off, 1 on)");
        c->opt_sky = (int)v;
        return RT_OK;
    case RT_OPT_DEFER_ROOTS:
        if (v < 0 || v > 1) return fail(RT_ERR_INVALID, "defer roots out of range (0 off, 1 on)");
        c->opt_defer_roots = (int)v;
        return RT_OK;
    default: return fail(RT_ERR_INVALID, "unknown option");
    }
}

int rt_ctx_get_option(rt_ctx* c, int key, int64_t* v)
{
    if (!c || !v) return fail(RT_ERR_INVALID, "null argument");
    switch (key) {
    case RT_OPT_TRACE_BUF_BYTES: *v = (int64_t)c->sample_buf_cap; return RT_OK;
    case RT_OPT_BATCH_OVERLAP: *v = c->opt.overlap; return RT_OK;
    case RT_OPT_BLOCK_SAMPLES: *v = c->opt.block_samples; return RT_OK;
    case RT_OPT_BLOCK_CHUNKS: *v = c->opt.block_chunks; return RT_OK;
    case RT_OPT_EXTRA_FEATURES: *v = c->opt.extra_features; return RT_OK;
    case RT_OPT_HOIST: *v = c->opt_hoist; return RT_OK;
    case RT_OPT_POOL_RING: *v = c->opt.ring; return RT_OK;
    case RT_OPT_COMM_DIRECT: *v = c->opt_comm_direct; return RT_OK;
    case RT_OPT_AUTO_DEAL_ORDER: *v = c->opt_deal; return RT_OK;
    case RT_OPT_PRIMARY_CANDIDATES: *v = c->opt_primary; return RT_OK;
    case RT_OPT_PRIMARY_CANDIDATES_K: *v = c->opt_primary_k; return RT_OK;
    case RT_OPT_SKIP_SKY_TILES: *v = c->opt_sky; return RT_OK;
    case RT_OPT_DEFER_ROOTS: *v = c->opt_defer_roots; return RT_OK;
    default: return fail(RT_ERR_INVALID, "unknown option");
    }
}

int rt_ctx_set_schedule(rt_ctx* c, int schedule)
{
    if (c && schedule == 4)   // the wavefront schedule of ABI v4 (rejected, scripts/experiments/r05_wavefront.patch)
        return fail(RT_ERR_UNSUPPORTED, "schedule 4 (wavefront) was removed: 2.3x slower than the pool on C4 (DESIGN.md 5.7)");
    if (!c || schedule < RT_SCHED_CHUNKS || schedule > RT_SCHED_AUTO) return fail(RT_ERR_INVALID, "bad schedule");
    c->opt.schedule = schedule;
    return RT_OK;
}

int rt_device_eval(rt_ctx* c, int fn, const double* x, const double* y, const double* z, double* out, int n)
{
    if (!c || !x || !out || n < 0 || fn < 0 || fn > 13) return fail(RT_ERR_INVALID, "bad argument");
    if (n == 0) return RT_OK;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf blk;
    const size_t b = (size_t)n * sizeof(double);
    HIP_TRY(blk.alloc(4 * b));
    double* const d = blk.as<double>();
    hipError_t e = hipMemcpy(d, x, b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, y ? y : x, b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * n, z ? z : x, b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtk::launch_eval(fn, d, d + n, d + 2 * n, d + 3 * n, n, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d + 3 * n, b, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "rt_device_eval");
    return RT_OK;
}

}  // extern "C"
