// abi.cpp — the extern "C" boundary (include/rt/rt_abi.h). No exception and no
// C++ type crosses it; every entry point returns RT_OK or a negative RT_ERR_*.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <limits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rt/rt_abi.h"
#include "adaptive_criterion.hpp"
#include "atrous.hpp"
#include "ctx_internal.hpp"
#include "deal_cache.hpp"
#include "denoise.hpp"
#include "features_kernel.hpp"
#include "launch_plan.hpp"
#include "scene_lower.hpp"
#include "scene_model.hpp"
#include "trace_kernel.hpp"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg)
{
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what)
{
    return fail(RT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t e_ = (expr);                         \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// device slots for launch params (a ring: a render's params stay intact while later
// renders are enqueued behind it on the same stream)
constexpr int kParamSlots = 16;

}  // namespace

struct rt_world {
    explicit rt_world(uint64_t seed) : w(seed) {}
    rtw::World w;
};

constexpr int kCounters = 32;  // count_work counters (trace_device.hpp: the trace kernels' epilogues; rt_last_counters)

struct rt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    void* scene_buf = nullptr;
    size_t scene_bytes = 0;
    rtk::SceneDev S{};
    bool has_scene = false;
    double* partial = nullptr;
    size_t partial_cap = 0;
    void* out_buf = nullptr;
    size_t out_cap = 0;
    unsigned long long* counters = nullptr;
    rtk::KParams* params = nullptr;     // ring of kParamSlots device copies of the launch params
    int param_slot = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    // Cross-stream ordering: the scratch buffers (partial, work counter, acc_tmp, counters,
    // params ring, staging) are per context, so work enqueued on a new stream must wait for
    // everything the context enqueued on the previous one. ev_done is recorded after each
    // enqueue; a call on another stream first makes that stream wait for it.
    hipEvent_t ev_done = nullptr;
    hipStream_t last_stream = nullptr;
    bool any_enqueued = false;
    bool pending_stats = false;
    bool pending_counts = false;
    rt_stats stats{};
    rt_adaptive_stats astats{};         // the last rt_render_adaptive (rt_adaptive_last_stats)
    rt_denoise_stats dstats{};          // the last rt_denoise (rt_denoise_last_stats)
    hipEvent_t ev_dn[2] = {nullptr, nullptr};   // around its kernel
    bool pending_dn = false;            // its kernel_ms is still to be read from the events
    rt_features_stats fstats{};         // the last rt_render_features (rt_features_last_stats)
    hipEvent_t ev_ft[3] = {nullptr, nullptr, nullptr};   // before its trace launches, after them, after its reductions
    bool pending_ft = false;            // its times are still to be read from the events
    rt_atrous_stats wstats{};           // the last rt_denoise_atrous (rt_atrous_last_stats)
    hipEvent_t ev_at[2] = {nullptr, nullptr};   // around its level kernels
    bool pending_at = false;            // its kernel_ms is still to be read from the events
    rtk::AtrousRec* atrous_buf = nullptr;   // its state scratch between levels (grown on demand)
    size_t atrous_cap = 0;              //   bytes
    // what a render's launch plan is made from (launch_plan.hpp): the uploaded scene, the device, the switches
    rtp::SceneFacts scene;
    rtp::DeviceFacts dev;
    rtp::Options opt;
    int opt_comm_direct = 1;            // RT_OPT_COMM_DIRECT: a world-1 rt_render_gather renders straight into the frame
    double* ring = nullptr;             // RT_OPT_POOL_RING's per-wave record rings (kPoolRing blocks per wave)
    size_t ring_cap = 0;
    unsigned long long raw_counters[kCounters] = {};   // the last count_work render's counters (rt_last_counters)
    uint32_t* tile_order = nullptr;     // rt_ctx_set_tile_order: tile shards' position -> raster tile (device)
    int64_t tile_order_n = 0;           //   its length (0: raster order)
    unsigned long long* tile_cost = nullptr;   // count_work pool renders: lane-cycles per raster tile
    int64_t tile_cost_cap = 0;          //   tiles allocated
    int64_t tile_cost_n = 0;            //   tiles of the last count_work render (rt_last_tile_costs)
    int opt_hoist = 1;                  // RT_OPT_HOIST: test a huge root-child leaf before the walk (pre_leaf)
    size_t sample_buf_cap = (size_t)32 << 30;  // RT_OPT_TRACE_BUF_BYTES: bound of the trace-output buffer
    unsigned* work = nullptr;           // pool / item schedules: work-block counters (one per overlapped batch),
    size_t work_stride = rtk::kDealTable;   //   work_stride words apart: each one's deal table and tile costs follow it
    // Overlapped buffer batches (RT_OPT_BATCH_OVERLAP): batch k traces on tstream[k & 1] into half k & 1
    // of the trace-output buffer while the caller's stream reduces batch k - 1
    hipStream_t tstream[2] = {nullptr, nullptr};
    hipEvent_t ev_in = nullptr, ev_tr[2] = {nullptr, nullptr}, ev_rd[2] = {nullptr, nullptr};
    double* acc_tmp = nullptr;          // running sums when a render takes several buffer batches
    size_t acc_tmp_cap = 0;
    // RT_OPT_AUTO_DEAL_ORDER (deal_cache.hpp): whole-frame pool renders dealt in the cost order the
    // product kernel measured on the first render of a (scene upload, camera, frame)
    int opt_deal = rtd::kAuto;
    uint64_t upload_gen = 0;            // scene uploads so far (the cache's key)
    rtd::DealCache deal;
    int64_t deal_cap = 0;               // tiles the deal tables behind the work counters hold (trace_kernel.hpp, kDealTable)
    int64_t last_deal_n = 0;            // tiles of the order the last render was dealt in (0: raster; rt_last_deal_order)
};

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
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&c->ev[i]);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipMalloc((void**)&c->counters, kCounters * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&c->params, kParamSlots * sizeof(rtk::KParams));
    if (e == hipSuccess) e = hipMalloc((void**)&c->work, 2 * rtk::kDealTable * sizeof(unsigned));
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipStreamCreateWithFlags(&c->tstream[i], hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->ev_tr[i], hipEventDisableTiming);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&c->ev_rd[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreate(&c->ev_dn[i]);
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&c->ev_ft[i]);
    for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreate(&c->ev_at[i]);
    if (e != hipSuccess) {
        rt_ctx_destroy(c);
        return hip_fail(e, "rt_ctx_create");
    }
    *out = c;
    return RT_OK;
}

void rt_ctx_destroy(rt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev_done && c->any_enqueued) (void)hipEventSynchronize(c->ev_done);  // work on a caller's stream
    (void)hipFree(c->scene_buf);
    (void)hipFree(c->partial);
    (void)hipFree(c->ring);
    (void)hipFree(c->out_buf);
    (void)hipFree(c->counters);
    (void)hipFree(c->tile_order);
    (void)hipFree(c->tile_cost);
    (void)hipFree(c->params);
    (void)hipFree(c->work);
    (void)hipFree(c->acc_tmp);
    (void)hipFree(c->atrous_buf);
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    if (c->ev_done) (void)hipEventDestroy(c->ev_done);
    for (int i = 0; i < 2; ++i) {
        if (c->tstream[i]) (void)hipStreamSynchronize(c->tstream[i]);
        if (c->tstream[i]) (void)hipStreamDestroy(c->tstream[i]);
        if (c->ev_tr[i]) (void)hipEventDestroy(c->ev_tr[i]);
        if (c->ev_rd[i]) (void)hipEventDestroy(c->ev_rd[i]);
    }
    if (c->ev_in) (void)hipEventDestroy(c->ev_in);
    for (auto& e : c->ev_dn)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : c->ev_ft)
        if (e) (void)hipEventDestroy(e);
    for (auto& e : c->ev_at)
        if (e) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// ---- world -------------------------------------------------------------------
int rt_world_create(uint64_t scene_seed, rt_world** out)
{
    if (!out) return fail(RT_ERR_INVALID, "null out");
    *out = new (std::nothrow) rt_world(scene_seed);
    return *out ? RT_OK : fail(RT_ERR_OOM, "rt_world");
}
void rt_world_destroy(rt_world* w) { delete w; }

#define CHECK_WORLD(w, o)                                              \
    do {                                                               \
        if (!(w) || !(o)) return fail(RT_ERR_INVALID, "null argument"); \
    } while (0)

static rtw::V3 vec(const double* a) { return rtw::v3(a[0], a[1], a[2]); }

int rt_world_texture_solid(rt_world* w, double r, double g, double b, int* o)
{
    CHECK_WORLD(w, o);
    *o = w->w.texture_solid(rtw::v3(r, g, b));
    return RT_OK;
}
int rt_world_texture_checker(rt_world* w, const double even[3], const double odd[3], int* o)
{
    CHECK_WORLD(w, o);
    if (!even || !odd) return fail(RT_ERR_INVALID, "null color");
    *o = w->w.texture_checker(vec(even), vec(odd));
    return RT_OK;
}
int rt_world_texture_noise(rt_world* w, double scale, int* o)
{
    CHECK_WORLD(w, o);
    *o = w->w.texture_noise(scale);
    return RT_OK;
}
int rt_world_texture_image(rt_world* w, const uint8_t* rgb, int width, int height, int* o)
{
    CHECK_WORLD(w, o);
    if (width < 0 || height < 0 || (!rgb && width * height > 0)) return fail(RT_ERR_INVALID, "bad image");
    *o = w->w.texture_image(rgb, width, height);
    return RT_OK;
}

int rt_world_material_lambertian(rt_world* w, int tex, int* o)
{
    CHECK_WORLD(w, o);
    if (!w->w.valid_texture(tex)) return fail(RT_ERR_INVALID, "bad texture id");
    *o = w->w.lambertian(tex);
    return RT_OK;
}
int rt_world_material_metal(rt_world* w, const double albedo[3], double fuzz, int* o)
{
    CHECK_WORLD(w, o);
    if (!albedo) return fail(RT_ERR_INVALID, "null albedo");
    *o = w->w.metal(vec(albedo), fuzz);
    return RT_OK;
}
int rt_world_material_dielectric(rt_world* w, double ir, int* o)
{
    CHECK_WORLD(w, o);
    *o = w->w.dielectric(ir);
    return RT_OK;
}
int rt_world_material_diffuse_light(rt_world* w, int tex, int* o)
{
    CHECK_WORLD(w, o);
    if (!w->w.valid_texture(tex)) return fail(RT_ERR_INVALID, "bad texture id");
    *o = w->w.diffuse_light(tex);
    return RT_OK;
}
int rt_world_material_isotropic(rt_world* w, int tex, int* o)
{
    CHECK_WORLD(w, o);
    if (!w->w.valid_texture(tex)) return fail(RT_ERR_INVALID, "bad texture id");
    *o = w->w.isotropic(tex);
    return RT_OK;
}

int rt_world_sphere(rt_world* w, int mat, const double c[3], double r, int* o)
{
    CHECK_WORLD(w, o);
    if (!c || !w->w.valid_material(mat)) return fail(RT_ERR_INVALID, "bad sphere");
    *o = w->w.sphere(mat, vec(c), r);
    return RT_OK;
}
int rt_world_moving_sphere(rt_world* w, int mat, const double c0[3], const double c1[3], double t0, double t1,
                           double r, int* o)
{
    CHECK_WORLD(w, o);
    if (!c0 || !c1 || !w->w.valid_material(mat)) return fail(RT_ERR_INVALID, "bad moving sphere");
    *o = w->w.moving_sphere(mat, vec(c0), vec(c1), t0, t1, r);
    return RT_OK;
}
int rt_world_rect(rt_world* w, int axis, int mat, double a0, double a1, double b0, double b1, double k, int* o)
{
    CHECK_WORLD(w, o);
    if (axis < 0 || axis > 2 || !w->w.valid_material(mat)) return fail(RT_ERR_INVALID, "bad rect");
    rtw::HKind kind = axis == 0 ? rtw::HKind::XYRect : axis == 1 ? rtw::HKind::XZRect : rtw::HKind::YZRect;
    *o = w->w.rect(kind, mat, a0, a1, b0, b1, k);
    return RT_OK;
}
int rt_world_box(rt_world* w, const double mn[3], const double mx[3], int mat, int* o)
{
    CHECK_WORLD(w, o);
    if (!mn || !mx || !w->w.valid_material(mat)) return fail(RT_ERR_INVALID, "bad box");
    *o = w->w.box(vec(mn), vec(mx), mat);
    return RT_OK;
}
int rt_world_translate(rt_world* w, int child, const double off[3], int* o)
{
    CHECK_WORLD(w, o);
    if (!off || !w->w.valid_hittable(child)) return fail(RT_ERR_INVALID, "bad translate");
    *o = w->w.translate(child, vec(off));
    return RT_OK;
}
int rt_world_rotate_y(rt_world* w, int child, double angle, int* o)
{
    CHECK_WORLD(w, o);
    if (!w->w.valid_hittable(child)) return fail(RT_ERR_INVALID, "bad rotate_y");
    *o = w->w.rotate_y(child, angle);
    return RT_OK;
}
int rt_world_constant_medium(rt_world* w, int boundary, double density, int phase, int* o)
{
    CHECK_WORLD(w, o);
    if (!w->w.valid_hittable(boundary) || !w->w.valid_material(phase)) return fail(RT_ERR_INVALID, "bad medium");
    *o = w->w.constant_medium(boundary, density, phase);
    return RT_OK;
}
int rt_world_bvh(rt_world* w, const int* ids, int n, double t0, double t1, int* o)
{
    CHECK_WORLD(w, o);
    if (!ids || n <= 0) return fail(RT_ERR_INVALID, "empty bvh list");
    std::vector<int> list(ids, ids + n);
    for (int id : list)
        if (!w->w.valid_hittable(id)) return fail(RT_ERR_INVALID, "bad id in bvh list");
    *o = w->w.bvh(list, 0, n, t0, t1);
    return RT_OK;
}
int rt_world_push(rt_world* w, int id)
{
    if (!w || !w->w.valid_hittable(id)) return fail(RT_ERR_INVALID, "bad hittable id");
    w->w.push(id);
    return RT_OK;
}

int rt_world_build_scene(rt_world* w, int scene_id, const uint8_t* img, int iw, int ih)
{
    if (!w) return fail(RT_ERR_INVALID, "null world");
    int rc = rtw::build_scene(w->w, scene_id, img, iw, ih);
    if (rc) return fail(rc, "unknown scene id or missing image texture");
    return RT_OK;
}

// Same structure probe as the oracle's orc_scene_info (leaves through BVHs,
// instances and media; span-1 duplicates counted once).
static void count_leaves(const rtw::World& w, int id, int& n, double& cs)
{
    const rtw::HNode& h = w.nodes[id];
    switch (h.kind) {
    case rtw::HKind::BvhNode:
        count_leaves(w, h.left, n, cs);
        if (h.right != h.left) count_leaves(w, h.right, n, cs);
        return;
    case rtw::HKind::Translate: case rtw::HKind::RotateY: case rtw::HKind::ConstantMedium:
        count_leaves(w, h.ptr, n, cs);
        return;
    default: {
        n++;
        double cy1 = h.kind == rtw::HKind::MovingSphere ? h.c1.y : 0.0;
        double rad = (h.kind == rtw::HKind::Sphere || h.kind == rtw::HKind::MovingSphere) ? h.radius : 0.0;
        double k = (h.kind == rtw::HKind::XYRect || h.kind == rtw::HKind::XZRect || h.kind == rtw::HKind::YZRect) ? h.k : 0.0;
        double by = h.kind == rtw::HKind::Box ? h.bmax.y : 0.0;
        double c0x = (h.kind == rtw::HKind::Sphere || h.kind == rtw::HKind::MovingSphere) ? h.c0.x : 0.0;
        double c0y = (h.kind == rtw::HKind::Sphere || h.kind == rtw::HKind::MovingSphere) ? h.c0.y : 0.0;
        double c0z = (h.kind == rtw::HKind::Sphere || h.kind == rtw::HKind::MovingSphere) ? h.c0.z : 0.0;
        cs += c0x + 2.0 * c0y + 3.0 * c0z + rad + k + by + cy1;
        return;
    }
    }
}

int rt_world_info_get(const rt_world* w, rt_world_info* out)
{
    if (!w || !out) return fail(RT_ERR_INVALID, "null argument");
    int n = 0;
    double cs = 0.0;
    for (int id : w->w.hittables) count_leaves(w->w, id, n, cs);
    for (const rtw::Material& m : w->w.materials) {
        double tex_c0y = m.tex >= 0 ? w->w.textures[m.tex].c0.y : 0.0;
        double albedo_x = m.kind == RT_MAT_METAL ? m.albedo.x : 0.0;
        cs += 0.5 * (albedo_x + tex_c0y + m.fuzz + m.ir);
    }
    out->n_hittables = (int32_t)w->w.hittables.size();
    out->n_materials = (int32_t)w->w.materials.size();
    out->n_leaf_prims = n;
    out->n_media = w->w.n_media;
    out->checksum = cs;
    return RT_OK;
}

// ---- camera -----------------------------------------------------------------------
int rt_camera_new(const double look_from[3], const double look_at[3], const double vup[3], double vfov,
                  double aspect, double aperture, double focus_dist, double t0, double t1, rt_camera* out)
{
    if (!look_from || !look_at || !vup || !out) return fail(RT_ERR_INVALID, "null argument");
    *out = rtw::camera_new(vec(look_from), vec(look_at), vec(vup), vfov, aspect, aperture, focus_dist, t0, t1);
    return RT_OK;
}

int rt_scene_preset_get(int scene_id, rt_scene_preset* out)
{
    if (!out) return fail(RT_ERR_INVALID, "null out");
    rtw::Preset p;
    if (!rtw::scene_preset(scene_id, p)) return fail(RT_ERR_INVALID, "unknown scene id");
    auto put = [](double* d, rtw::V3 a) { d[0] = a.x; d[1] = a.y; d[2] = a.z; };
    put(out->look_from, p.look_from);
    put(out->look_at, p.look_at);
    put(out->background, p.background);
    out->vfov = p.vfov;
    out->aperture = 0.1;     // main.rs:469
    out->focus_dist = 10.0;  // main.rs:312
    out->time0 = 0.0;
    out->time1 = 1.0;
    out->default_width = p.width;
    out->default_spp = p.spp;
    out->default_aspect = p.aspect;
    return RT_OK;
}

int rt_scene_camera(int scene_id, int width, int height, rt_camera* cam, double bg[3])
{
    if (!cam || width < 1 || height < 1) return fail(RT_ERR_INVALID, "bad argument");
    rtw::Preset p;
    if (!rtw::scene_preset(scene_id, p)) return fail(RT_ERR_INVALID, "unknown scene id");
    *cam = rtw::camera_new(p.look_from, p.look_at, rtw::v3(0.0, 1.0, 0.0), p.vfov, (double)width / (double)height,
                           0.1, 10.0, 0.0, 1.0);
    if (bg) {
        bg[0] = p.background.x;
        bg[1] = p.background.y;
        bg[2] = p.background.z;
    }
    return RT_OK;
}

// ---- lowering + upload ---------------------------------------------------------------
int rt_world_set_build_option(rt_world* w, int key, double v)
{
    if (!w) return fail(RT_ERR_INVALID, "null world");
    if (!std::isfinite(v)) return fail(RT_ERR_INVALID, "build option value not finite");
    rtw::BuildOptions& b = w->w.build;
    const int iv = v < 0 ? -1 : (int)std::min(v, 1e6);
    switch (key) {
    case RT_BUILD_C_ISECT: b.c_isect = v > 0 ? v : 0.0; return RT_OK;
    case RT_BUILD_MAX_LEAF: b.max_leaf = std::max(iv, 0); return RT_OK;
    case RT_BUILD_FORCE_LEAF: b.force_leaf = std::max(iv, 0); return RT_OK;
    case RT_BUILD_ROOT_LEAF: b.root_leaf = iv; return RT_OK;
    case RT_BUILD_SPLIT_BOX_PAIRS: b.split_box_pairs = iv; return RT_OK;
    case RT_BUILD_SPLIT_BLAS_PAIRS: b.split_blas_pairs = iv; return RT_OK;
    default: return fail(RT_ERR_INVALID, "unknown build option");
    }
}

int rt_world_flatten(rt_world* w, int accel, const rt_scene_soa** soa_out)
{
    if (!w || !soa_out) return fail(RT_ERR_INVALID, "null argument");
    std::string err;
    int rc = rtw::flatten(w->w, accel, err);
    if (rc) return fail(rc, err);
    *soa_out = &w->w.flat.soa;
    return RT_OK;
}

int rt_scene_validate(const rt_scene_soa* s, int32_t* tlas_depth, int32_t* blas_depth)
{
    if (!s) return fail(RT_ERR_INVALID, "null argument");
    int t = 0, b = 0, n = 0;
    std::string err;
    const int rc = rtl::validate(*s, t, b, n, err);
    if (rc) return fail(rc, err);
    if (tlas_depth) *tlas_depth = t;
    if (blas_depth) *blas_depth = b;
    return RT_OK;
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
    if (c->any_enqueued) HIP_TRY(hipEventSynchronize(c->ev_done));  // renders still reading the scene
    if (total > c->scene_bytes) {
        (void)hipFree(c->scene_buf);
        c->scene_buf = nullptr;
        c->scene_bytes = 0;
        HIP_TRY(hipMalloc(&c->scene_buf, total));
        c->scene_bytes = total;
    }
    char* base = (char*)c->scene_buf;
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
using rtp::auto_chunk;
using rtp::bad_geometry;
using rtp::Layout;
using rtp::layout_of;
using rtp::row_block_of;

static int grow(rt_ctx* c, hipStream_t stream, double*& buf, size_t& cap, size_t need, bool* oom = nullptr)
{
    if (need <= cap) return RT_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    (void)hipFree(buf);
    buf = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc((void**)&buf, need);
    if (e == hipErrorOutOfMemory && oom) {   // the caller retries with a smaller batch
        (void)hipGetLastError();
        buf = nullptr;
        *oom = true;
        return RT_ERR_HIP;
    }
    HIP_TRY(e);
    cap = need;
    return RT_OK;
}

// Where a sample range's per-pixel sums go: added to acc (n_px x 3 f64), or (acc null)
// written as sum * scale to out (f32 / f64).
struct Sink {
    double* acc = nullptr;
    void* out = nullptr;
    bool f64 = true;
    double scale = 1.0;
    // rt_render_adaptive's passes (acc and out unused): a tile shard under the call's own tile
    // order (moments->order), on the per-sample buffer whatever the context's schedule, reduced by
    // the moments kernel into the call's frame-layout accumulators; n_done = samples per pixel
    // of the shard's tiles once this range is in
    const rtk::AdaptiveFrame* moments = nullptr;
    int n_done = 0;
};

// The launch params of a sample range, all but what the plan and the batch loop set (block sizes,
// ring, sample range, work blocks). Fails on a context tile order that is not the frame's.
static int fill_kparams(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const Layout& lay, int chunk,
                        const Sink& sink, int64_t img_tiles, rtk::KParams& K)
{
    std::memset(&K, 0, sizeof K);
    K.cam = *cam;
    for (int i = 0; i < 3; ++i) K.bg[i] = p->background[i];
    K.scale_m11 = rt_uniform_incl_scale(-1.0, 1.0);
    K.scale_time = rt_uniform_incl_scale(cam->time0, cam->time1);
    K.wm1 = (double)p->width - 1.0;
    K.hm1 = (double)p->height - 1.0;
    K.inv_wm1 = 1.0 / K.wm1;
    K.inv_hm1 = 1.0 / K.hm1;
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
        K.tile_order = c->tile_order;
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
static int deal_setup(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rtp::Plan& pl, bool adaptive_pass,
                      int64_t img_tiles, hipStream_t stream, rtk::KParams& K)
{
    c->last_deal_n = 0;
    const bool ok = rtk::deal_variant(pl.variant) && rtd::eligible(*p, pl.schedule, adaptive_pass);
    const rtd::Decision d = c->deal.next(c->opt_deal, ok, rtd::key_of(c->upload_gen, *cam, *p), img_tiles);
    const size_t n = (size_t)img_tiles;
    if (d.measure) {
        if (img_tiles > c->deal_cap) {   // (a key's first render: no work on the context's streams reads them)
            HIP_TRY(hipStreamSynchronize(stream));
            const size_t stride = rtk::kDealTable + 2 * n;
            unsigned* w = nullptr;
            const hipError_t e = hipMalloc((void**)&w, 2 * stride * sizeof(unsigned));
            if (e != hipSuccess) {
                c->deal.drop();
                return hip_fail(e, "deal order table");
            }
            (void)hipFree(c->work);
            c->work = w;
            c->work_stride = stride;
            c->deal_cap = img_tiles;
        }
        std::vector<uint32_t> raster(n);
        for (size_t i = 0; i < n; ++i) raster[i] = (uint32_t)i;
        for (int h = 0; h < 2; ++h) {
            unsigned* t = c->work + h * c->work_stride + rtk::kDealTable;
            HIP_TRY(hipMemcpyAsync(t, raster.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemsetAsync(t + n, 0, n * sizeof(unsigned), stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));   // (raster is pageable and local)
        K.tile_major = rtk::kDealMeasure;
    }
    if (d.build) {
        std::vector<uint32_t> part(2 * n);
        hipError_t e = hipSuccess;
        for (int h = 0; h < 2 && e == hipSuccess; ++h)
            e = hipMemcpyAsync(part.data() + h * n, c->work + h * c->work_stride + rtk::kDealTable + n, n * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) {
            c->deal.fail_build();
            return hip_fail(e, "deal order: tile costs");
        }
        std::vector<uint64_t> costs(n);   // (overlapped batches count on both counters' tables)
        for (size_t i = 0; i < n; ++i) costs[i] = (uint64_t)part[i] + part[n + i];
        const std::vector<uint32_t>& order = c->deal.finish_build(costs.data());
        for (int h = 0; h < 2 && e == hipSuccess; ++h)
            e = hipMemcpyAsync(c->work + h * c->work_stride + rtk::kDealTable, order.data(), n * sizeof(uint32_t),
                               hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);   // (the pageable copy's source is the cache's, kept; the sync is cheap here)
        if (e != hipSuccess) {
            c->deal.fail_build();
            return hip_fail(e, "deal order: upload");
        }
    }
    if (d.ordered) {
        K.tile_major = rtk::kDealOrdered;
        c->last_deal_n = img_tiles;
    }
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
    c->pending_stats = true;
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
static int run_range(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int s_begin, int s_end, int chunk,
                     hipStream_t stream, const Sink& sink)
{
    const Layout lay = layout_of(p);
    const long long n_px = (long long)lay.rows * lay.w;
    if (n_px == 0 || s_end <= s_begin) {
        // an empty shard (rt_rows_in_shard / rt_tiles_in_shard 0: a rank past the tile count)
        // or an empty sample range: nothing to trace or write; the events still bracket the
        // (empty) work so rt_last_stats resolves
        for (int i = 0; i < 3; ++i) HIP_TRY(hipEventRecord(c->ev[i], stream));
        write_stats(c, rtp::Plan{}, chunk, 0, false);
        c->last_deal_n = 0;
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
    // the plan, and its buffers: an attempt whose trace output (or ring) does not fit the device
    // is planned again without the ring, or under half the bound (this render only: the
    // context's bound stays, so a later render on it uses the memory freed since)
    rtp::Retry retry{c->sample_buf_cap, true};
    rtp::Plan pl;
    for (;;) {
        pl = rtp::plan(c->scene, c->dev, c->opt, rq, retry);
        if (pl.err) return fail(pl.err, pl.err_msg);
        rc = grow(c, stream, c->acc_tmp, c->acc_tmp_cap, pl.acc_bytes);
        if (rc) return rc;
        bool oom = false;
        rc = grow(c, stream, c->partial, c->partial_cap, pl.partial_bytes, &oom);
        if (rc == RT_OK && pl.ring) {
            rc = grow(c, stream, c->ring, c->ring_cap, pl.ring_bytes, &oom);
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
    double* const open = pl.open_chunk ? c->acc_tmp : nullptr;
    double* const acc = !pl.own_total ? sink.acc : pl.open_chunk ? c->acc_tmp + pl.px * 3 : c->acc_tmp;
    rtk::SceneDev S = c->S;
    S.n_lds_nodes = pl.n_lds_nodes;
    S.n_lds_materials = pl.n_lds_materials;
    S.n_lds_textures = pl.n_lds_textures;
    S.n_lds_blas = pl.n_lds_blas;
    S.seed_stage_bytes = (int32_t)pl.seed_stage_bytes;
    K.block_chunks = pl.block_chunks;
    K.block_samples = pl.block_samples;
    K.ring_waves = pl.ring_waves;
    int waves_per_simd = 0;
    rtk::LaunchOpts o;
    o.features = pl.features;
    o.slab32 = pl.slab32;
    o.lds_stack = pl.lds_stack;
    o.count = rq.count_work;
    o.pool = pl.schedule;
    o.f32 = pl.f32;
    o.waves_per_simd = &waves_per_simd;
    const rtk::SampleTiles tiles{lay.w, lay.rows, (lay.w + 7) / 8, pl.f32};
    rc = deal_setup(c, cam, p, pl, sink.moments != nullptr, img_tiles, stream, K);
    if (rc) return rc;

    if (pl.own_total) HIP_TRY(hipMemsetAsync(acc, 0, pl.px_bytes, stream));
    if (rq.count_work) {
        HIP_TRY(hipMemsetAsync(c->counters, 0, kCounters * sizeof(unsigned long long), stream));
        if (img_tiles > c->tile_cost_cap) {   // (a render's first use: no work on the context's streams reads it)
            HIP_TRY(hipStreamSynchronize(stream));
            (void)hipFree(c->tile_cost);
            c->tile_cost = nullptr;
            c->tile_cost_cap = 0;
            HIP_TRY(hipMalloc((void**)&c->tile_cost, (size_t)img_tiles * sizeof(unsigned long long)));
            c->tile_cost_cap = img_tiles;
        }
        HIP_TRY(hipMemsetAsync(c->tile_cost, 0, (size_t)img_tiles * sizeof(unsigned long long), stream));
        K.tile_cost = c->tile_cost;
        // (the pool kernels count them; the chunk schedule does not)
        c->tile_cost_n = pl.schedule == RT_SCHED_POOL || pl.schedule == RT_SCHED_ITEMS ? img_tiles : 0;
    }
    HIP_TRY(hipEventRecord(c->ev[0], stream));
    // overlapped batches: both trace streams start after everything enqueued on `stream` so far
    if (pl.overlap) {
        HIP_TRY(hipEventRecord(c->ev_in, stream));
        for (int i = 0; i < 2; ++i) HIP_TRY(hipStreamWaitEvent(c->tstream[i], c->ev_in, 0));
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
            K.n_work_blocks = (unsigned)K.tiles_x * (unsigned)K.tiles_y * n_groups;
            K.deal_div = K.tile_major ? n_groups : (unsigned)K.tiles_x * (unsigned)K.tiles_y;
        }
        // batch bi's buffer half, trace stream and work counter (one of each per overlapped batch)
        const int h = pl.overlap ? (bi & 1) : 0;
        double* buf = c->partial + (size_t)h * (pl.half_bytes / sizeof(double));
        hipStream_t ts = pl.overlap ? c->tstream[h] : stream;
        K.ring = pl.ring ? c->ring + (size_t)h * (pl.ring_one_bytes / sizeof(double)) : nullptr;   // one ring per trace stream
        if (pl.overlap && bi >= 2) HIP_TRY(hipStreamWaitEvent(ts, c->ev_rd[h], 0));   // batch bi - 2 reduced: half free
        rtk::KParams* dK = c->params + c->param_slot;
        c->param_slot = (c->param_slot + 1) % kParamSlots;
        HIP_TRY(hipMemcpyAsync(dK, &K, sizeof K, hipMemcpyHostToDevice, ts));
        HIP_TRY(rtk::launch_trace(S, K, dK, buf, c->counters, c->work + h * c->work_stride, o, ts));
        if (bi == pl.n_batches - 1) HIP_TRY(hipEventRecord(c->ev[1], ts));
        if (pl.overlap) {   // reduce in batch order on `stream`, after this batch's trace
            HIP_TRY(hipEventRecord(c->ev_tr[h], ts));
            HIP_TRY(hipStreamWaitEvent(stream, c->ev_tr[h], 0));
        }
        if (sink.moments) {
            HIP_TRY(rtk::launch_adaptive_moments(buf, *sink.moments, K.tiles_x, b1 - b0, chunk,
                                                 (int)(((long long)b0 - s_begin) % chunk), bi == pl.n_batches - 1,
                                                 sink.n_done, stream));
        } else if (!pl.per_sample) {
            if (acc) HIP_TRY(rtk::launch_accumulate(buf, acc, n_px, K.n_chunks, stream));
            else HIP_TRY(rtk::launch_reduce(buf, sink.out, sink.f64, n_px, K.n_chunks, sink.scale, stream));
        } else if (!open) {
            HIP_TRY(rtk::launch_reduce_samples(buf, sink.out, sink.f64, tiles, b1 - b0, chunk, sink.scale, stream));
        } else {
            HIP_TRY(rtk::launch_reduce_samples_carry(buf, acc, open, tiles, b1 - b0, chunk,
                                                     (int)(((long long)b0 - s_begin) % chunk), bi == pl.n_batches - 1,
                                                     stream));
        }
        if (pl.overlap) HIP_TRY(hipEventRecord(c->ev_rd[h], stream));
    }
    if (pl.own_total)  // resolve the running sums: 0.0 + sum, times scale, as one batch does
        HIP_TRY(rtk::launch_reduce(acc, sink.out, sink.f64, n_px, 1, sink.scale, stream));
    HIP_TRY(hipEventRecord(c->ev[2], stream));
    write_stats(c, pl, chunk, waves_per_simd, rq.count_work);
    return RT_OK;
}

// Orders work about to be enqueued on `stream` after everything this context enqueued on
// another stream before (the context's scratch buffers are shared between its renders).
static int begin_on(rt_ctx* c, hipStream_t stream)
{
    if (c->any_enqueued && stream != c->last_stream) HIP_TRY(hipStreamWaitEvent(stream, c->ev_done, 0));
    return RT_OK;
}
static int end_on(rt_ctx* c, hipStream_t stream)
{
    HIP_TRY(hipEventRecord(c->ev_done, stream));
    c->last_stream = stream;
    c->any_enqueued = true;
    return RT_OK;
}
// begin_on ... end_on around every call that enqueues: once begin_on has run, end_on runs on
// every way out, an early error return included — work already queued on `stream` before the
// error still reads the context's buffers, and the next call on another stream must wait
// for it (ev_done, last_stream), not for the call before
struct StreamScope {
    rt_ctx* c;
    hipStream_t stream;
    bool open = false;
    StreamScope(rt_ctx* c_, hipStream_t s_) : c(c_), stream(s_) {}
    int begin()
    {
        const int rc = begin_on(c, stream);
        open = rc == RT_OK;
        return rc;
    }
    int end()
    {
        open = false;
        return end_on(c, stream);
    }
    ~StreamScope()
    {
        if (open) (void)end_on(c, stream);
    }
};

// Device buffer for a host-bound result (grown on demand).
static int out_staging(rt_ctx* c, hipStream_t stream, size_t out_bytes, void*& dev_out)
{
    if (out_bytes > c->out_cap) {
        HIP_TRY(hipStreamSynchronize(stream));  // ordered after every earlier use (begin_on)
        (void)hipFree(c->out_buf);
        c->out_buf = nullptr;
        c->out_cap = 0;
        HIP_TRY(hipMalloc(&c->out_buf, std::max<size_t>(out_bytes, 16)));
        c->out_cap = std::max<size_t>(out_bytes, 16);
    }
    dev_out = c->out_buf;
    return RT_OK;
}

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
        rc = out_staging(c, stream, out_bytes, dev_out);
        if (rc) return rc;
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
    double* sums = nullptr;             // device, n_px x 3
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
    if (e == hipSuccess) e = hipMalloc((void**)&a->sums, bytes);
    if (e == hipSuccess) e = hipMemset(a->sums, 0, bytes);
    if (e != hipSuccess) {
        (void)hipFree(a->sums);
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
    (void)hipFree(a->sums);
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
    sink.acc = a->sums;
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
    HIP_TRY(hipMemcpy(sums, a->sums, (size_t)a->n_px * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_accum_set(rt_accum* a, const double* sums, int64_t samples_done)
{
    if (!a || !sums) return fail(RT_ERR_INVALID, "null argument");
    if (samples_done < 0 || samples_done > 0x7fffffffLL) return fail(RT_ERR_INVALID, "bad sample count");
    HIP_TRY(hipSetDevice(a->ctx->device));
    HIP_TRY(hipStreamSynchronize(a->last_stream));
    HIP_TRY(hipMemcpy(a->sums, sums, (size_t)a->n_px * 3 * sizeof(double), hipMemcpyHostToDevice));
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
        rc = out_staging(c, stream, out_bytes, dev_out);
        if (rc) return rc;
    }
    // one "chunk" holding the running sums: 0.0 + sum = sum, then * (1/divisor) as rt_render
    HIP_TRY(rtk::launch_reduce(a->sums, dev_out, out_format == RT_OUT_F64, a->n_px, 1, 1.0 / divisor, stream));
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

namespace {
struct DeviceBlock {   // one allocation for a call's device state, freed on every way out
    void* p = nullptr;
    ~DeviceBlock() { (void)hipFree(p); }
};
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair()
    {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};
}  // namespace

int rt_render_adaptive(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_adaptive_params* ap,
                       const rt_adaptive_out* out)
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

    // device state: [sum | sum_open | q | q_open | tile_error | se map (host-bound only)] f64, then
    // [tile_spp | order A | order B | counts] u32; zeroed: the sums start from 0.0
    const size_t hw = (size_t)W * (size_t)H, nt = (size_t)n_tiles;
    const bool own_se = out->stderr_map && !on_dev;
    const size_t n_f64 = 8 * hw + nt + (own_se ? hw : 0), n_u32 = 3 * nt + 2;
    DeviceBlock blk;
    HIP_TRY(hipMalloc(&blk.p, n_f64 * sizeof(double) + n_u32 * sizeof(uint32_t)));
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
    {
        std::vector<uint32_t> raster(nt);
        for (size_t i = 0; i < nt; ++i) raster[i] = (uint32_t)i;
        HIP_TRY(hipMemcpyAsync(order[0], raster.data(), nt * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));   // (raster is read until the copy is done)
    }
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.a));
    HIP_TRY(hipEventCreate(&ev.b));

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
        rc = run_range(c, cam, &rp, done, end, chunk, stream, sink);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(ev.a, stream));
        HIP_TRY(rtk::launch_adaptive_compact(order[cur], order[cur ^ 1], F.tile_error, n_tiles, n_stopped, ap->threshold,
                                             end >= p->spp, counts, stream));
        uint32_t h_counts[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(h_counts, counts, sizeof h_counts, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(ev.b, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float t_trace = 0, t_moments = 0, t_classify = 0;
        HIP_TRY(hipEventElapsedTime(&t_trace, c->ev[0], c->ev[1]));
        HIP_TRY(hipEventElapsedTime(&t_moments, c->ev[1], c->ev[2]));
        HIP_TRY(hipEventElapsedTime(&t_classify, ev.a, ev.b));
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
        rc = out_staging(c, stream, mean_bytes, dev_mean);
        if (rc) return rc;
    }
    HIP_TRY(rtk::launch_adaptive_resolve(F.sum, F.q, F.tile_spp, dev_mean, p->out_format == RT_OUT_F64, se_dev, W, H, stream));
    const hipMemcpyKind kind = on_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!on_dev) HIP_TRY(hipMemcpyAsync(out->mean, dev_mean, mean_bytes, kind, stream));
    if (own_se) HIP_TRY(hipMemcpyAsync(out->stderr_map, se_dev, hw * sizeof(double), kind, stream));
    if (out->tile_spp) HIP_TRY(hipMemcpyAsync(out->tile_spp, F.tile_spp, nt * sizeof(uint32_t), kind, stream));
    if (out->tile_error) HIP_TRY(hipMemcpyAsync(out->tile_error, F.tile_error, nt * sizeof(double), kind, stream));
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
    c->pending_stats = false;
    c->pending_counts = false;
    c->astats = as;
    return RT_OK;
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
    rc = grow(c, stream, c->partial, c->partial_cap, (size_t)batch * chunk_bytes);
    if (rc) return rc;
    if (n_batches > 1) {
        rc = grow(c, stream, c->acc_tmp, c->acc_tmp_cap, chunk_bytes);
        if (rc) return rc;
    }
    // host-bound frames: staged [albedo | normal | depth] in the context's output buffer
    const size_t px = (size_t)n_px;
    double *d_albedo = out->albedo, *d_normal = out->normal, *d_depth = out->depth;
    if (!on_dev) {
        void* stage = nullptr;
        rc = out_staging(c, stream, 7 * px * sizeof(double), stage);
        if (rc) return rc;
        double* s = (double*)stage;
        d_albedo = out->albedo ? s : nullptr;
        d_normal = out->normal ? s + 3 * px : nullptr;
        d_depth = out->depth ? s + 6 * px : nullptr;
    }

    const int64_t img_tiles = (int64_t)((W + 7) / 8) * ((H + 7) / 8);
    rtk::KParams K;
    rc = fill_kparams(c, cam, &rp, lay, chunk, Sink{}, img_tiles, K);
    if (rc) return rc;
    rtk::SceneDev S = c->S;
    S.n_lds_nodes = pl.n_lds_nodes;
    S.n_lds_materials = pl.n_lds_materials;
    S.n_lds_textures = pl.n_lds_textures;
    S.n_lds_blas = pl.n_lds_blas;
    rtk::LaunchOpts o;
    o.features = pl.features;
    o.slab32 = pl.slab32;
    o.lds_stack = pl.lds_stack;
    o.count = 0;
    o.pool = RT_SCHED_CHUNKS;
    o.f32 = 0;

    HIP_TRY(hipEventRecord(c->ev_ft[0], stream));
    for (int bi = 0; bi < n_batches; ++bi) {
        const int c0 = bi * batch, c1 = std::min(n_chunks, c0 + batch);
        K.sample_begin = c0 * chunk;
        K.spp = (int)std::min<long long>(p->spp, (long long)c1 * chunk);
        K.n_chunks = c1 - c0;
        rtk::KParams* dK = c->params + c->param_slot;
        c->param_slot = (c->param_slot + 1) % kParamSlots;
        HIP_TRY(hipMemcpyAsync(dK, &K, sizeof K, hipMemcpyHostToDevice, stream));
        HIP_TRY(rtk::launch_features(S, K, dK, c->partial, o, stream));
        if (bi == n_batches - 1) HIP_TRY(hipEventRecord(c->ev_ft[1], stream));
        HIP_TRY(rtk::launch_reduce_features(c->partial, c->acc_tmp, d_albedo, d_normal, d_depth, n_px, K.n_chunks, bi == 0,
                                            bi == n_batches - 1, 1.0 / (double)p->spp, stream));
    }
    HIP_TRY(hipEventRecord(c->ev_ft[2], stream));
    c->fstats = rt_features_stats{};
    c->fstats.samples = (uint64_t)n_px * (uint64_t)p->spp;
    c->fstats.variant_features = (int32_t)pl.variant;
    c->fstats.spp_chunk = chunk;
    c->pending_ft = true;
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
    if (c->pending_ft) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipEventSynchronize(c->ev_ft[2]));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, c->ev_ft[0], c->ev_ft[1]));
        HIP_TRY(hipEventElapsedTime(&b, c->ev_ft[1], c->ev_ft[2]));
        c->fstats.kernel_ms = a;
        c->fstats.reduce_ms = b;
        c->pending_ft = false;
    }
    *out = c->fstats;
    return RT_OK;
}

// ---- variance-guided NL-means (rt_abi.h: the filter; denoise_kernel.hip; denoise_host.cpp) -------
namespace {
// rt_denoise_host lives in denoise_host.cpp, which links without this file: its error text comes
// through a hook
[[maybe_unused]] const bool g_denoise_sink_set =(rtk::denoise_error_sink = [](const char* msg) { g_last_error = msg; }, true);
}  // namespace

int rt_denoise_guided(rt_ctx* c, const rt_denoise_params* p, const void* mean, const double* stderr_map,
                      const rt_denoise_guides* g, void* out)
{
    if (!c) return fail(RT_ERR_INVALID, "null argument");
    if (const char* bad = rtk::denoise_check(p, mean, stderr_map, out)) return fail(RT_ERR_INVALID, bad);
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::denoise_guides_check(g, G)) return fail(RT_ERR_INVALID, bad);
    const bool f64 = p->format == RT_OUT_F64, on_dev = p->on_device != 0;
    const size_t hw = (size_t)p->width * (size_t)p->height;
    const size_t frame_bytes = hw * 3 * (f64 ? 8 : 4), se_bytes = hw * sizeof(double);

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;

    // host pointers: the frame, the map, the result and the guides staged in one device block of the call's own
    DeviceBlock blk;
    const void* d_mean = mean;
    const double* d_se = stderr_map;
    void* d_out = out;
    if (!on_dev) {
        const size_t off_se = align_up(frame_bytes, 256), off_out = off_se + align_up(se_bytes, 256);
        const size_t g3 = align_up(hw * 3 * sizeof(double), 256), g1 = align_up(se_bytes, 256);
        const size_t off_ga = off_out + align_up(frame_bytes, 256), off_gn = off_ga + (G.albedo ? g3 : 0);
        const size_t off_gz = off_gn + (G.normal ? g3 : 0);
        HIP_TRY(hipMalloc(&blk.p, off_gz + (G.depth ? g1 : 0) + 256));
        d_mean = blk.p;
        d_se = (const double*)((char*)blk.p + off_se);
        d_out = (char*)blk.p + off_out;
        HIP_TRY(hipMemcpyAsync(blk.p, mean, frame_bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync((void*)d_se, stderr_map, se_bytes, hipMemcpyHostToDevice, stream));
        auto stage = [&](const double*& guide, size_t off, size_t bytes) {
            if (!guide) return hipSuccess;
            void* d = (char*)blk.p + off;
            const hipError_t e = hipMemcpyAsync(d, guide, bytes, hipMemcpyHostToDevice, stream);
            guide = (const double*)d;
            return e;
        };
        HIP_TRY(stage(G.albedo, off_ga, hw * 3 * sizeof(double)));
        HIP_TRY(stage(G.normal, off_gn, hw * 3 * sizeof(double)));
        HIP_TRY(stage(G.depth, off_gz, se_bytes));
    }
    HIP_TRY(hipEventRecord(c->ev_dn[0], stream));
    HIP_TRY(rtk::launch_denoise(d_mean, d_se, d_out, f64, p->width, p->height, p->radius, p->patch, p->k, G, stream));
    HIP_TRY(hipEventRecord(c->ev_dn[1], stream));
    c->dstats = rt_denoise_stats{};
    c->dstats.radius = p->radius;
    c->dstats.patch = p->patch;
    c->dstats.lds_bytes = rtk::denoise_lds_bytes(p->radius, p->patch);
    c->pending_dn = true;
    if (!on_dev) HIP_TRY(hipMemcpyAsync(out, d_out, frame_bytes, hipMemcpyDeviceToHost, stream));
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
    if (c->pending_dn) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipEventSynchronize(c->ev_dn[1]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_dn[0], c->ev_dn[1]));
        c->dstats.kernel_ms = ms;
        c->pending_dn = false;
    }
    *out = c->dstats;
    return RT_OK;
}

// ---- variance-guided a-trous wavelet filter (rt_abi.h: the filter; atrous_kernel.hip; atrous_host.cpp)
namespace {
[[maybe_unused]] const bool g_atrous_sink_set = (rtk::atrous_error_sink = [](const char* msg) { g_last_error = msg; }, true);
}  // namespace

// The context's state scratch for a call that needs `bytes` of it (grown on demand).
static int atrous_scratch(rt_ctx* c, hipStream_t stream, size_t bytes, rtk::AtrousRec*& buf)
{
    if (bytes > c->atrous_cap) {
        HIP_TRY(hipStreamSynchronize(stream));  // ordered after every earlier use (begin_on)
        (void)hipFree(c->atrous_buf);
        c->atrous_buf = nullptr;
        c->atrous_cap = 0;
        HIP_TRY(hipMalloc((void**)&c->atrous_buf, bytes));
        c->atrous_cap = bytes;
    }
    buf = bytes ? c->atrous_buf : nullptr;
    return RT_OK;
}

int rt_denoise_atrous(rt_ctx* c, const rt_atrous_params* p, const void* mean, const double* stderr_map,
                      const rt_denoise_guides* g, void* out, double* stderr_out)
{
    if (!c) return fail(RT_ERR_INVALID, "null argument");
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::atrous_check(p, mean, stderr_map, g, out, stderr_out, G)) return fail(RT_ERR_INVALID, bad);
    const bool f64 = p->format == RT_OUT_F64, on_dev = p->on_device != 0;
    const size_t hw = (size_t)p->width * (size_t)p->height;
    const size_t frame_bytes = hw * 3 * (f64 ? 8 : 4), se_bytes = hw * sizeof(double);
    const size_t scratch_bytes = (size_t)rtk::atrous_state_buffers(p->levels) * hw * sizeof(rtk::AtrousRec);

    HIP_TRY(hipSetDevice(c->device));
    hipStream_t stream = p->stream ? (hipStream_t)p->stream : c->stream;
    StreamScope scope(c, stream);
    int rc = scope.begin();
    if (rc) return rc;
    rtk::AtrousRec* scratch = nullptr;
    rc = atrous_scratch(c, stream, scratch_bytes, scratch);
    if (rc) return rc;

    // host pointers: the frame, the map, the results and the guides staged in one device block of the call's own
    DeviceBlock blk;
    const void* d_mean = mean;
    const double* d_se = stderr_map;
    void* d_out = out;
    double* d_se_out = stderr_out;
    if (!on_dev) {
        const size_t g3 = align_up(hw * 3 * sizeof(double), 256), g1 = align_up(se_bytes, 256);
        const size_t off_se = align_up(frame_bytes, 256), off_out = off_se + g1;
        const size_t off_so = off_out + align_up(frame_bytes, 256), off_ga = off_so + (stderr_out ? g1 : 0);
        const size_t off_gn = off_ga + (G.albedo ? g3 : 0), off_gz = off_gn + (G.normal ? g3 : 0);
        HIP_TRY(hipMalloc(&blk.p, off_gz + (G.depth ? g1 : 0) + 256));
        d_mean = blk.p;
        d_se = (const double*)((char*)blk.p + off_se);
        d_out = (char*)blk.p + off_out;
        if (stderr_out) d_se_out = (double*)((char*)blk.p + off_so);
        HIP_TRY(hipMemcpyAsync(blk.p, mean, frame_bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync((void*)d_se, stderr_map, se_bytes, hipMemcpyHostToDevice, stream));
        auto stage = [&](const double*& guide, size_t off, size_t bytes) {
            if (!guide) return hipSuccess;
            void* d = (char*)blk.p + off;
            const hipError_t e = hipMemcpyAsync(d, guide, bytes, hipMemcpyHostToDevice, stream);
            guide = (const double*)d;
            return e;
        };
        HIP_TRY(stage(G.albedo, off_ga, hw * 3 * sizeof(double)));
        HIP_TRY(stage(G.normal, off_gn, hw * 3 * sizeof(double)));
        HIP_TRY(stage(G.depth, off_gz, se_bytes));
    }
    HIP_TRY(hipEventRecord(c->ev_at[0], stream));
    HIP_TRY(rtk::launch_atrous(d_mean, d_se, d_out, d_se_out, f64, p->width, p->height, p->levels, p->sigma_l,
                               p->demodulate ? G.albedo : nullptr, G, scratch, stream));
    HIP_TRY(hipEventRecord(c->ev_at[1], stream));
    c->wstats = rt_atrous_stats{};
    c->wstats.levels = p->levels;
    c->wstats.scratch_bytes = (int64_t)scratch_bytes;
    c->pending_at = true;
    if (!on_dev) {
        HIP_TRY(hipMemcpyAsync(out, d_out, frame_bytes, hipMemcpyDeviceToHost, stream));
        if (stderr_out) HIP_TRY(hipMemcpyAsync(stderr_out, d_se_out, se_bytes, hipMemcpyDeviceToHost, stream));
    }
    rc = scope.end();
    if (rc) return rc;
    if (!on_dev) HIP_TRY(hipStreamSynchronize(stream));   // (the block is freed once its copies are done)
    return RT_OK;
}

int rt_atrous_last_stats(rt_ctx* c, rt_atrous_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    if (c->pending_at) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipEventSynchronize(c->ev_at[1]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_at[0], c->ev_at[1]));
        c->wstats.kernel_ms = ms;
        c->pending_at = false;
    }
    *out = c->wstats;
    return RT_OK;
}

int rt_last_stats(rt_ctx* c, rt_stats* out)
{
    if (!c || !out) return fail(RT_ERR_INVALID, "null argument");
    if (c->pending_stats) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipEventSynchronize(c->ev[2]));
        float a = 0, b = 0;
        HIP_TRY(hipEventElapsedTime(&a, c->ev[0], c->ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, c->ev[1], c->ev[2]));
        c->stats.kernel_ms = a;
        c->stats.reduce_ms = b;
        if (c->pending_counts) {
            unsigned long long h[kCounters];
            HIP_TRY(hipMemcpy(h, c->counters, sizeof h, hipMemcpyDeviceToHost));
            c->stats.casts = h[0];
            c->stats.node_visits = h[1];
            c->stats.prim_tests = h[2];
            c->stats.cycles_camera = h[3];
            c->stats.cycles_trace = h[4];
            c->stats.cycles_shade = h[5];
            c->stats.wave_steps = h[6];
            c->stats.wave_node_steps = h[7];
            c->stats.cycles_nodes = h[8];
            c->stats.cycles_leaves = h[9];
            c->stats.wave_leaf_steps = h[10];
            c->stats.camera_lanes = h[11];
            c->stats.camera_steps = h[12];
            c->stats.shade_lanes = h[13];
            c->stats.shade_steps = h[14];
            for (int i = 0; i < kCounters; ++i) c->raw_counters[i] = h[i];
        } else {
            c->stats.casts = c->stats.node_visits = c->stats.prim_tests = 0;
            c->stats.cycles_camera = c->stats.cycles_trace = c->stats.cycles_shade = 0;
            c->stats.wave_steps = c->stats.wave_node_steps = 0;
            c->stats.cycles_nodes = c->stats.cycles_leaves = 0;
            c->stats.wave_leaf_steps = c->stats.camera_lanes = c->stats.camera_steps = 0;
            c->stats.shade_lanes = c->stats.shade_steps = 0;
            for (int i = 0; i < kCounters; ++i) c->raw_counters[i] = 0;
        }
        c->pending_stats = false;
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
    if (m > 0) HIP_TRY(hipMemcpy(out, c->tile_cost, (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost));
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
    (void)hipFree(c->tile_order);
    c->tile_order = nullptr;
    c->tile_order_n = 0;
    if (n == 0) return RT_OK;
    HIP_TRY(hipMalloc((void**)&c->tile_order, (size_t)n * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(c->tile_order, order, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
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

// ---- output ---------------------------------------------------------------------------------
// write_color (math.rs:119-131) of one f64 channel summed over spp samples: scale = 1.0/spp,
// sqrt(x * scale), clamp to [0, 0.999] (NaN passes through, math.rs:282-286), 256 * c with
// Rust's saturating `as i32` (NaN -> 0). All in f64, as the reference: with rt_render's
// RT_OUT_F64 mean (sum * (1/spp)) and spp = 1 this is write_color(spp) of the sums bit for bit.
static inline int write_color_f64(double x, double scale)
{
    const double r = std::sqrt(x * scale);
    const double c = r < 0.0 ? 0.0 : r > 0.999 ? 0.999 : r;
    return (int)rt_sat_i32(256.0 * c);
}

int rt_write_color(const double* rgb, int samples_per_pixel, int64_t n, int32_t* out)
{
    if (!rgb || !out || n < 0 || samples_per_pixel < 1) return fail(RT_ERR_INVALID, "bad argument");
    const double scale = 1.0 / (double)samples_per_pixel;
    for (int64_t i = 0; i < 3 * n; ++i) out[i] = write_color_f64(rgb[i], scale);
    return RT_OK;
}

int rt_write_ppm_f64(const double* rgb, int samples_per_pixel, int width, int height, const char* path)
{
    if (!rgb || !path || width < 1 || height < 1 || samples_per_pixel < 1) return fail(RT_ERR_INVALID, "bad argument");
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(RT_ERR_INVALID, std::string("cannot open ") + path);
    const double scale = 1.0 / (double)samples_per_pixel;           // math.rs:120
    std::fprintf(f, "P3\n%d %d\n255\n\n", width, height);          // main.rs:472 (println! adds the blank line)
    for (int j = height - 1; j >= 0; --j)                          // main.rs:591-596: rows top to bottom
        for (int i = 0; i < width; ++i) {
            const double* px = rgb + ((size_t)j * width + i) * 3;
            std::fprintf(f, "%d %d %d\n", write_color_f64(px[0], scale), write_color_f64(px[1], scale),
                         write_color_f64(px[2], scale));
        }
    if (std::fclose(f) != 0) return fail(RT_ERR_INVALID, std::string("cannot write ") + path);
    return RT_OK;
}

// The f32 frame's writer (RT_OUT_F32 renders, the f32 mode): the mean is rounded to f32
// before the sqrt, so a channel whose 256*sqrt(mean) lies within ~1e-5 of an integer may
// differ by one from the reference's f64 write_color; rt_write_ppm_f64 is the exact one.
int rt_write_ppm(const float* mean, int width, int height, const char* path)
{
    if (!mean || !path || width < 1 || height < 1) return fail(RT_ERR_INVALID, "bad argument");
    FILE* f = std::fopen(path, "wb");
    if (!f) return fail(RT_ERR_INVALID, std::string("cannot open ") + path);
    std::fprintf(f, "P3\n%d %d\n255\n\n", width, height);  // main.rs:472 (println! adds the blank line)
    auto to_byte = [](double x) {                           // math.rs:119-131
        double r = std::sqrt(x);
        double c = r < 0.0 ? 0.0 : r > 0.999 ? 0.999 : r;   // clamp (NaN passes through)
        return (int)rt_sat_i32(256.0 * c);                  // `as i32`: NaN -> 0
    };
    for (int j = height - 1; j >= 0; --j)                   // main.rs:591-596
        for (int i = 0; i < width; ++i) {
            const float* px = mean + ((size_t)j * width + i) * 3;
            std::fprintf(f, "%d %d %d\n", to_byte(px[0]), to_byte(px[1]), to_byte(px[2]));
        }
    std::fclose(f);
    return RT_OK;
}

// ---- self test ----------------------------------------------------------------------------------
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
    double* d = nullptr;
    const size_t b = (size_t)n * sizeof(double);
    HIP_TRY(hipMalloc((void**)&d, 4 * b));
    hipError_t e = hipMemcpy(d, x, b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, y ? y : x, b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * n, z ? z : x, b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtk::launch_eval(fn, d, d + n, d + 2 * n, d + 3 * n, n, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d + 3 * n, b, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "rt_device_eval");
    return RT_OK;
}

}  // extern "C"

// ---- what comm.cpp reads of a context (ctx_internal.hpp) ---------------------------------------
namespace rtx {
int fail(int code, const std::string& msg) { return ::fail(code, msg); }
int hip_fail(hipError_t e, const char* what) { return ::hip_fail(e, what); }
int ctx_device(const rt_ctx* c) { return c->device; }
hipStream_t ctx_stream(const rt_ctx* c) { return c->stream; }
const uint32_t* ctx_tile_order(const rt_ctx* c, int64_t* n)
{
    *n = c->tile_order_n;
    return c->tile_order;
}
int ctx_schedule(const rt_ctx* c) { return c->opt.schedule; }
int ctx_precision(const rt_ctx* c) { return c->opt.precision; }
bool ctx_comm_direct(const rt_ctx* c) { return c->opt_comm_direct != 0; }
}  // namespace rtx
