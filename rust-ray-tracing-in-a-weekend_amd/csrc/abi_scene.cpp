// abi_scene.cpp — the entry points of include/rt/rt_abi.h that touch no context: the world
// builders, cameras and scene presets, flattening and validation, and the frame writers. As at
// every entry point, no exception and no C++ type crosses the boundary; each returns RT_OK or a
// negative RT_ERR_*.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <new>
#include <string>
#include <vector>

#include "rt/rt_abi.h"
#include "rt/rt_numerics.h"
#include "ctx_internal.hpp"
#include "primary_candidates.hpp"
#include "scene_lower.hpp"
#include "scene_model.hpp"

struct rt_world {
    explicit rt_world(uint64_t seed) : w(seed) {}
    rtw::World w;
};

extern "C" {

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
    // MovingSphere::center divides by t1 - t0 (hittable.rs:556-558): no centre, and no box, without it
    if (!std::isfinite(t0) || !std::isfinite(t1) || t0 == t1)
        return fail(RT_ERR_INVALID, "moving sphere: t0 and t1 must be finite and different");
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
    case RT_BUILD_TIME0: b.time0 = v; return RT_OK;
    case RT_BUILD_TIME1: b.time1 = v; return RT_OK;
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

// The primary-candidate table (primary_candidates.hpp) of a flattened scene, built on the host over
// the tables an upload would give the device (rtl::lower with the pre-leaf hoist): the host twin of
// what a render builds when RT_OPT_PRIMARY_CANDIDATES is on.
int rt_primary_candidates_host(const rt_scene_soa* s, const rt_camera* cam, int width, int height, int k_max,
                               uint16_t* records, rt_primary_candidates_info* info)
{
    if (!s || !cam || !records || width < 1 || height < 1 || k_max < 1) return fail(RT_ERR_INVALID, "bad argument");
    rtl::Lowered L;
    std::string err;
    const int rc = rtl::lower(*s, true, L, err);
    if (rc) return fail(rc, err);
    static_assert(sizeof(rtpc::Record) == 8 * sizeof(uint16_t), "a record is 8 uint16");
    const rtpc::TableStats st = rtpc::build_host(L.nodes.data(), L.leaf_prims.data(), s->tlas_root, *cam, width, height, k_max,
                                                 reinterpret_cast<rtpc::Record*>(records));
    if (info) {
        info->pixels = st.pixels;
        info->flagged = st.flagged;
        info->candidates = st.candidates;
        info->max_candidates = st.max_candidates;
        info->slots = rtpc::kSlots;
    }
    return RT_OK;
}

// The all-sky tile flags of that table (primary_candidates.hpp, tile_all_sky): the host twin of what
// a render builds beside the table when RT_OPT_SKIP_SKY_TILES is on.
int rt_primary_sky_tiles_host(const rt_scene_soa* s, const rt_camera* cam, int width, int height, int k_max, uint8_t* flags,
                              int64_t* count)
{
    if (!flags || width < 1 || height < 1) return fail(RT_ERR_INVALID, "bad argument");
    std::vector<rtpc::Record> table((size_t)width * (size_t)height);
    const int rc = rt_primary_candidates_host(s, cam, width, height, k_max, reinterpret_cast<uint16_t*>(table.data()), nullptr);
    if (rc) return rc;
    const int64_t n = rtpc::sky_tiles_host(table.data(), width, height, flags);
    if (count) *count = n;
    return RT_OK;
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

}  // extern "C"
