// lower_dump.cpp — what rtl::lower (csrc/scene_lower.cpp) makes of a fixed list of scenes, one
// JSON line per case: every scalar of rtl::Lowered, the kernel variant its features select, and
// a 64-bit FNV-1a hash of each of its four tables (over the named fields, never struct padding).
// Links scene_model.cpp, flatten.cpp, bvh_build.cpp and scene_lower.cpp (tests/test_lowering.py
// LOWERING_SOURCES) and nothing from HIP; built with ASan and UBSan and compared with
// tests/golden/lowering.json by tests/test_lowering.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "rt/rt_abi.h"
#include "scene_features.hpp"
#include "scene_lower.hpp"
#include "scene_model.hpp"

namespace {

using rtw::HKind;
using rtw::v3;
using rtw::World;

struct Fnv {
    uint64_t h = 14695981039346656037ull;
    template <class T>
    void add(const T& v)
    {
        unsigned char b[sizeof(T)];
        std::memcpy(b, &v, sizeof(T));
        for (unsigned char c : b) h = (h ^ c) * 1099511628211ull;
    }
    template <class T, size_t N>
    void add(const T (&a)[N])
    {
        for (const T& v : a) add(v);
    }
};

uint64_t hash_prims(const std::vector<rt_prim>& t)
{
    Fnv f;
    for (const rt_prim& p : t) f.add(p.kind), f.add(p.mat), f.add(p.a), f.add(p.b), f.add(p.p);
    return f.h;
}
uint64_t hash_nodes(const std::vector<rt_bvh_node>& t)
{
    Fnv f;
    for (const rt_bvh_node& n : t) f.add(n.lo0), f.add(n.hi0), f.add(n.lo1), f.add(n.hi1), f.add(n.child);
    return f.h;
}
uint64_t hash_instances(const std::vector<rt_instance>& t)
{
    Fnv f;
    for (const rt_instance& in : t) {
        f.add(in.n_ops), f.add(in.child_kind), f.add(in.child), f.add(in.pad), f.add(in.op_kind);
        for (const auto& row : in.op) f.add(row);
    }
    return f.h;
}

void dump(const char* name, const rt_scene_soa& s, bool hoist = true)
{
    rtl::Lowered L;
    std::string err;
    const int rc = rtl::lower(s, hoist, L, err);
    std::printf("{\"case\": \"%s\", \"rc\": %d, \"err\": \"%s\", \"n_prims\": %d, \"n_prim_refs\": %d, \"n_nodes\": %d, "
                "\"n_instances\": %d",
                name, rc, err.c_str(), s.n_prims, s.n_prim_refs, s.n_nodes, s.n_instances);
    if (rc == RT_OK) {
        std::printf(", \"features\": %u, \"variant\": %u, \"tlas_depth\": %d, \"blas_depth\": %d, \"n_tlas_nodes\": %d, "
                    "\"n_blas_bfs\": %d, \"blas_base\": %d, \"stack_entries\": %d, \"stack16_ok\": %d, \"pre_leaf\": %d, "
                    "\"pre_root\": %d, \"pre_lo\": [%.9g, %.9g, %.9g], \"pre_hi\": [%.9g, %.9g, %.9g], \"has_lights\": %d, "
                    "\"has_spheres\": %d, \"pad_extent\": %.17g",
                    L.features, rtk::variant_features(L.features), L.tlas_depth, L.blas_depth, L.n_tlas_nodes,
                    L.n_blas_bfs, L.blas_base, L.stack_entries, L.stack16_ok, L.pre_leaf, L.pre_root, L.pre_lo[0],
                    L.pre_lo[1], L.pre_lo[2], L.pre_hi[0], L.pre_hi[1], L.pre_hi[2], L.has_lights, L.has_spheres,
                    L.pad_extent);
        std::printf(", \"inst_pad\": [");   // each instance's BLAS base slot
        for (size_t i = 0; i < L.instances.size(); ++i) std::printf(i ? ", %d" : "%d", L.instances[i].pad);
        std::printf("]");
        std::printf(", \"prims\": \"%016llx\", \"leaf_prims\": \"%016llx\", \"nodes\": \"%016llx\", \"instances\": \"%016llx\"",
                    (unsigned long long)hash_prims(L.prims), (unsigned long long)hash_prims(L.leaf_prims),
                    (unsigned long long)hash_nodes(L.nodes), (unsigned long long)hash_instances(L.instances));
    }
    std::printf("}\n");
}

// flattens w and dumps it; edit (optional) changes a copy of the tables first (scenes the
// flattener never produces) and returns false if it found nothing to edit
struct Tables {
    std::vector<rt_bvh_node> nodes;
    std::vector<rt_instance> instances;
    rt_scene_soa soa;
};
void dump_world(const char* name, World& w, int accel = RT_ACCEL_SAH, bool hoist = true,
                const std::function<bool(Tables&)>& edit = nullptr)
{
    std::string err;
    const int rc = rtw::flatten(w, accel, err);
    if (rc) {
        std::printf("{\"case\": \"%s\", \"flatten_rc\": %d, \"err\": \"%s\"}\n", name, rc, err.c_str());
        return;
    }
    if (!edit) return dump(name, w.flat.soa, hoist);
    Tables t{w.flat.nodes, w.flat.instances, w.flat.soa};
    t.soa.nodes = t.nodes.data();
    t.soa.instances = t.instances.data();
    if (!edit(t)) {
        std::printf("{\"case\": \"%s\", \"err\": \"nothing to edit\"}\n", name);
        return;
    }
    dump(name, t.soa, hoist);
}

// a 4 x 2 RGB gradient for the image textures
const uint8_t* gradient()
{
    static uint8_t px[4 * 2 * 3];
    for (int y = 0; y < 2; ++y)
        for (int x = 0; x < 4; ++x) {
            uint8_t* p = px + (y * 4 + x) * 3;
            p[0] = (uint8_t)(x * 85);
            p[1] = (uint8_t)(y * 255);
            p[2] = (uint8_t)(255 - x * 85);
        }
    return px;
}

int white(World& w) { return w.lambertian(w.texture_solid(v3(0.73, 0.73, 0.73))); }
int bvh(World& w, const std::vector<int>& ids) { return w.bvh(ids, 0, (int)ids.size(), 0.0, 1.0); }

// ---- the small worlds of tests/test_gpu_nesting.py --------------------------------------
void nested_world(World& w)
{
    const int wh = white(w);
    const int red = w.lambertian(w.texture_checker(v3(0.65, 0.05, 0.05), v3(0.9, 0.9, 0.9)));
    const int metal = w.metal(v3(0.8, 0.8, 0.9), 0.1);
    const int glass = w.dielectric(1.5);
    const int light = w.diffuse_light(w.texture_solid(v3(6.0, 6.0, 6.0)));
    const int phase = w.isotropic(w.texture_solid(v3(0.8, 0.8, 0.9)));
    w.push(w.sphere(wh, v3(0.0, -1000.0, 0.0), 1000.0));
    w.push(w.rect(HKind::XZRect, light, -2.0, 2.0, -2.0, 2.0, 6.0));
    const int inner = w.rotate_y(w.translate(w.box(v3(0, 0, 0), v3(0.8, 1.6, 0.8), red), v3(0.3, 0.0, 0.0)), 25.0);
    const int fog = w.constant_medium(w.sphere(wh, v3(-1.2, 0.7, 0.0), 0.7), 0.9, phase);
    const int group = bvh(w, {inner, fog, w.sphere(metal, v3(1.4, 0.5, 0.3), 0.5), w.sphere(glass, v3(0.2, 0.4, 1.3), 0.4)});
    w.push(w.translate(w.rotate_y(group, -30.0), v3(0.0, 0.0, -1.0)));
    const int smoke = w.constant_medium(
        w.translate(w.rotate_y(w.box(v3(0, 0, 0), v3(1, 1, 1), wh), 15.0), v3(-0.5, 0.0, -0.5)), 1.5, phase);
    w.push(w.translate(w.rotate_y(smoke, 40.0), v3(-2.5, 0.0, 1.5)));
    w.push(w.constant_medium(bvh(w, {w.sphere(wh, v3(2.6, 0.6, 1.8), 0.6), w.sphere(wh, v3(3.3, 0.6, 1.8), 0.6)}), 1.2, phase));
    std::vector<int> balls;
    for (int i = 0; i < 6; ++i) balls.push_back(w.sphere(wh, v3(0.4 * i, 0.25, 0.0), 0.2));
    w.push(w.translate(w.rotate_y(w.translate(bvh(w, balls), v3(-1.0, 0.0, 0.0)), 70.0), v3(1.5, 0.0, -3.0)));
}

void moving_world(World& w, double t0, double t1)
{
    const int wh = w.lambertian(w.texture_checker(v3(0.2, 0.3, 0.1), v3(0.9, 0.9, 0.9)));
    const int red = w.lambertian(w.texture_solid(v3(0.7, 0.1, 0.1)));
    const int metal = w.metal(v3(0.8, 0.8, 0.9), 0.2);
    w.push(w.sphere(wh, v3(0.0, -1000.0, 0.0), 1000.0));
    for (int i = 0; i < 5; ++i) {
        const rtw::V3 c0 = v3(-2.0 + i, 0.3, 0.2 * i);
        w.push(w.moving_sphere(i % 2 ? red : metal, c0, v3(c0.x, c0.y + 0.4, c0.z), t0, t1, 0.3));
    }
    w.push(w.moving_sphere(red, v3(0.5, 1.2, -1.0), v3(0.9, 1.2, -1.0), 0.0, 1.0, 0.4));
}

// n spheres in a cluster (the last one moving if asked)
std::vector<int> cluster(World& w, int mat, int n, double dx = 0.0, bool moving = false)
{
    std::vector<int> ids;
    for (int i = 0; i < n; ++i)
        ids.push_back(w.sphere(mat, v3(dx + 0.3 * (i % 8) - 1.0, 0.25 + 0.3 * (i / 8), 0.1 * (i % 2)), 0.14));
    if (moving) ids.push_back(w.moving_sphere(mat, v3(dx, 1.0, 0.0), v3(dx + 0.3, 1.2, 0.0), 0.0, 1.0, 0.3));
    return ids;
}

// Translate(RotateY(BVH of n spheres)) + a ground sphere, the final scene's cluster shape
void instanced_spheres(World& w, int n, bool moving)
{
    const int wh = white(w);
    w.push(w.translate(w.rotate_y(bvh(w, cluster(w, wh, n, 0.0, moving)), 25.0), v3(0.2, 0.0, -0.5)));
    w.push(w.sphere(wh, v3(0.0, -100.0, 0.0), 100.0));
}

void shared_blas(World& w, int n)
{
    const int wh = white(w);
    const int balls = bvh(w, cluster(w, wh, n));
    w.push(w.translate(w.rotate_y(balls, 30.0), v3(-0.8, 0.0, 0.0)));
    w.push(w.translate(balls, v3(1.0, 0.0, -0.6)));
    w.push(w.sphere(wh, v3(0.0, -100.0, 0.0), 100.0));
}

void two_blases(World& w)
{
    const int wh = white(w);
    w.push(w.translate(w.rotate_y(bvh(w, cluster(w, wh, 40)), 30.0), v3(-0.8, 0.0, 0.0)));
    w.push(w.translate(bvh(w, cluster(w, wh, 12, 4.0)), v3(1.0, 0.0, -0.6)));
    w.push(w.sphere(wh, v3(0.0, -100.0, 0.0), 100.0));
}

// a ground sphere and n small spheres on a grid (the spheres variant)
void sphere_field(World& w, int n)
{
    const int ground = w.lambertian(w.texture_checker(v3(0.2, 0.3, 0.1), v3(0.9, 0.9, 0.9)));
    const int mats[3] = {w.lambertian(w.texture_solid(v3(0.7, 0.2, 0.1))), w.metal(v3(0.8, 0.8, 0.9), 0.1), w.dielectric(1.5)};
    w.push(w.sphere(ground, v3(0.0, -1000.0, 0.0), 1000.0));
    const int side = (int)std::ceil(std::sqrt((double)n));
    for (int i = 0; i < n; ++i)
        w.push(w.sphere(mats[i % 3], v3(-6.0 + 12.0 * (i % side) / side, 0.12, -6.0 + 12.0 * (i / side) / side), 0.1));
}

// a sphere field at the top level and one instance over a BLAS of n_blas spheres
void field_and_instance(World& w, int n_top, int n_blas)
{
    sphere_field(w, n_top);
    w.push(w.translate(w.rotate_y(bvh(w, cluster(w, white(w), n_blas)), 25.0), v3(0.2, 2.0, -0.5)));
}

// which: 0 a rect, 1 a sphere under an instance, 2 a top-level sphere
void image_world(World& w, int which)
{
    const int wh = white(w);
    const int img = w.lambertian(w.texture_image(gradient(), 4, 2));
    w.push(w.sphere(wh, v3(0.0, -100.0, 0.0), 100.0));
    if (which == 0) w.push(w.rect(HKind::XYRect, img, -1.0, 1.0, 0.0, 2.0, -1.0));
    if (which == 1) w.push(w.translate(w.sphere(img, v3(0.0, 1.0, 0.0), 1.0), v3(1.0, 0.0, 0.0)));
    if (which == 2) w.push(w.sphere(img, v3(0.0, 1.0, 0.0), 1.0));
}

// ---- edits of the flattened tables -----------------------------------------------------
// What the reference's bounding_box does not bound (flatten.cpp's box invariant): spheres of
// negative radius, alone, concentric and under a rotate_y, and moving spheres whose shutter does
// not cover the ray times [0, 1], among enough spheres for the top level to have nodes; under
// an rt_world_bvh node instead when under_bvh.
void unbounded_by_reference(World& w, bool under_bvh)
{
    const int wh = white(w), glass = w.dielectric(1.5);
    std::vector<int> ids;
    for (int i = 0; i < 12; ++i) ids.push_back(w.sphere(i % 2 ? wh : glass, v3((double)i, 0.5, 0.0), 0.4));
    ids.push_back(w.sphere(glass, v3(14.0, 3.0, 0.0), -0.9));
    ids.push_back(w.sphere(glass, v3(3.0, 2.0, 1.0), 0.6));
    ids.push_back(w.sphere(glass, v3(3.0, 2.0, 1.0), -0.5));
    for (int i = 0; i < 6; ++i)
        ids.push_back(w.moving_sphere(wh, v3((double)i, 0.5, 2.0), v3((double)i, 1.5, 2.0), i % 2 ? 0.25 : 2.0, i % 2 ? 0.75 : 3.0, 0.3));
    if (under_bvh) {
        w.push(bvh(w, ids));
    } else {
        for (int id : ids) w.push(id);
        w.push(w.translate(w.rotate_y(w.sphere(wh, v3(0.5, 0.5, 0.0), -0.4), 135.0), v3(-3.0, 0.0, 0.0)));
    }
}

bool spheres_only(const rt_scene_soa& s, int ref)
{
    if (ref >= 0) return spheres_only(s, s.nodes[ref].child[0]) && spheres_only(s, s.nodes[ref].child[1]);
    const int code = ~ref;
    for (int j = code >> 5; j < (code >> 5) + (code & 31); ++j)
        if (s.prims[s.prim_refs[j]].kind > RT_PRIM_MOVING_SPHERE) return false;
    return true;
}
// the first BVH instance gets a TLAS subtree that holds only spheres as its child
bool point_instance_at_tlas(Tables& t)
{
    for (rt_instance& in : t.instances) {
        if (in.child_kind != RT_CHILD_BVH) continue;
        for (int i = 1; i < t.soa.n_tlas_nodes; ++i)
            if (spheres_only(t.soa, i)) {
                in.child = i;
                return true;
            }
    }
    return false;
}
// a second TLAS leaf is made to cover the slot of a BVH instance
bool reference_instance_twice(Tables& t)
{
    const rt_scene_soa& s = t.soa;
    auto holds_instance = [&](int ref) {
        const int code = ~ref;
        for (int j = code >> 5; ref < 0 && j < (code >> 5) + (code & 31); ++j) {
            const rt_prim& p = s.prims[s.prim_refs[j]];
            if (p.kind == RT_PRIM_INSTANCE && s.instances[p.a].child_kind == RT_CHILD_BVH) return true;
        }
        return false;
    };
    int with = 0;
    for (int i = 0; i < s.n_tlas_nodes && !with; ++i)
        for (int ch : t.nodes[(size_t)i].child)
            if (holds_instance(ch)) with = ch;
    for (int i = 0; i < s.n_tlas_nodes && with; ++i)
        for (int& ch : t.nodes[(size_t)i].child)
            if (ch < 0 && !holds_instance(ch)) {
                ch = with;
                return true;
            }
    return false;
}
// The flattener gives every instance its own copy of a BLAS; these make the first instance
// share the second one's instead (whose first slot is not 0): its root (which < 0), or the
// subtree under child `which` of that root (the one holding the BLAS's first slot has the same
// base; the other has a base of its own: no relative codes)
bool share_blas(Tables& t, int which)
{
    if (t.instances.size() < 2 || t.instances[0].child_kind != RT_CHILD_BVH || t.instances[1].child_kind != RT_CHILD_BVH)
        return false;
    const int root = t.instances[1].child;
    if (which >= 0 && (root < 0 || t.nodes[(size_t)root].child[which] < 0)) return false;
    t.instances[0].child = which < 0 ? root : t.nodes[(size_t)root].child[which];
    return true;
}
// Tables validate must refuse (rc != 0 and its message): the first instance over the top-level
// leaf, whose slots hold the instances themselves; a cycle in the second instance's BLAS
bool instance_over_instances(Tables& t)
{
    if (t.instances.empty() || t.instances[0].child_kind != RT_CHILD_BVH || t.soa.tlas_root >= 0) return false;
    t.instances[0].child = t.soa.tlas_root;
    return true;
}
bool cycle_in_second_blas(Tables& t)
{
    if (t.instances.size() < 2 || t.instances[1].child_kind != RT_CHILD_BVH) return false;
    const int root = t.instances[1].child;
    if (root < 0 || t.nodes[(size_t)root].child[0] < 0) return false;
    t.nodes[(size_t)t.nodes[(size_t)root].child[0]].child[1] = root;
    return true;
}

}  // namespace

int main()
{
    static const char* const accel_name[3] = {"sah", "linear", "median"};
    // the eight reference scenes
    for (int accel = 0; accel < 3; ++accel)
        for (int id = 0; id < 8; ++id) {
            if (accel != RT_ACCEL_SAH && id != 0 && id != 5 && id != 7) continue;
            World w(1);
            if (rtw::build_scene(w, id, gradient(), 4, 2)) return 1;
            const std::string name = "scene" + std::to_string(id) + "_" + accel_name[accel];
            dump_world(name.c_str(), w, accel);
            if (id == 0 && accel == RT_ACCEL_SAH) dump_world("scene0_sah_nohoist", w, accel, false);
        }
    {
        World w(5);
        nested_world(w);
        for (int accel = 0; accel < 3; ++accel) dump_world((std::string("nested_") + accel_name[accel]).c_str(), w, accel);
    }
    const double shutters[3][2] = {{0.0, 1.0}, {0.25, 0.75}, {-1.0, 2.0}};
    for (int i = 0; i < 3; ++i) {   // [0, 1]: the spheres variant; others: FEAT_SHUTTER
        World w(3);
        moving_world(w, shutters[i][0], shutters[i][1]);
        dump_world(("shutter_" + std::to_string(i)).c_str(), w);
    }
    for (int moving = 0; moving < 2; ++moving) {   // FEAT_NEST_MOVING: variant 4095; all static: 287
        World w(1);
        instanced_spheres(w, 6, moving != 0);
        dump_world(moving ? "instanced_moving" : "instanced_static", w);
    }
    for (int n : {3, 40}) {   // two instances of one BVH (a single leaf, a tree): lowered to a BLAS each ...
        World w(1);
        shared_blas(w, n);
        dump_world(("shared_blas_" + std::to_string(n)).c_str(), w);
        // ... and really sharing one: the same pad, its codes rewritten once
        dump_world(("shared_root_" + std::to_string(n)).c_str(), w, RT_ACCEL_SAH, true,
                   [](Tables& t) { return share_blas(t, -1); });
        if (n != 40) continue;
        dump_world("shared_subtree_0", w, RT_ACCEL_SAH, true, [](Tables& t) { return share_blas(t, 0); });
        dump_world("shared_subtree_1", w, RT_ACCEL_SAH, true, [](Tables& t) { return share_blas(t, 1); });
        // refused: a non-primitive under an instance, a cycle, and the first of the two when both are there
        dump_world("refused_nonprimitive", w, RT_ACCEL_SAH, true, instance_over_instances);
        dump_world("refused_cycle", w, RT_ACCEL_SAH, true, cycle_in_second_blas);
        dump_world("refused_nonprimitive_then_cycle", w, RT_ACCEL_SAH, true,
                   [](Tables& t) { return instance_over_instances(t) && cycle_in_second_blas(t); });
        dump_world("refused_bad_node", w, RT_ACCEL_SAH, true, [](Tables& t) {
            t.nodes[0].child[0] = t.soa.n_nodes;   // one past the node table
            return true;
        });
    }
    {   // two instances, two BLASes: a second nested walk, stack_entries is the sum
        World w(1);
        two_blases(w);
        dump_world("two_blases", w);
    }
    {   // an instance over a medium: FEAT_INST_MEDIUM, inst_boundary
        World w(1);
        const int wh = white(w), phase = w.isotropic(w.texture_solid(v3(0.8, 0.8, 0.9)));
        w.push(w.translate(w.constant_medium(w.sphere(wh, v3(0, 1, 0), 1.0), 0.9, phase), v3(1.0, 0.0, 0.0)));
        w.push(w.translate(w.rotate_y(bvh(w, cluster(w, wh, 12)), 25.0), v3(0.2, 0.0, -0.5)));
        w.push(w.sphere(wh, v3(0.0, -100.0, 0.0), 100.0));
        dump_world("instance_over_medium", w);
    }
    {   // a medium whose boundary is an instance: FEAT_MEDIUM_INST, inst_boundary
        World w(1);
        const int wh = white(w), phase = w.isotropic(w.texture_solid(v3(0.8, 0.8, 0.9)));
        w.push(w.constant_medium(w.translate(w.rotate_y(w.box(v3(0, 0, 0), v3(1, 1, 1), wh), 15.0), v3(-0.5, 0.0, -0.5)), 1.5, phase));
        w.push(w.translate(w.rotate_y(bvh(w, cluster(w, wh, 12)), 25.0), v3(0.2, 0.0, -0.5)));
        w.push(w.sphere(wh, v3(0.0, -100.0, 0.0), 100.0));
        dump_world("medium_instance_boundary", w);
    }
    {   // a medium bounded by an instance over a BVH that holds a moving sphere
        World w(1);
        const int wh = white(w), phase = w.isotropic(w.texture_solid(v3(0.8, 0.8, 0.9)));
        w.push(w.constant_medium(w.translate(bvh(w, cluster(w, wh, 5, 0.0, true)), v3(0.0, 0.5, 0.0)), 1.5, phase));
        w.push(w.sphere(wh, v3(0.0, -100.0, 0.0), 100.0));
        dump_world("medium_moving_boundary", w);
    }
    static const char* const image_name[3] = {"image_rect", "image_instanced_sphere", "image_top_sphere"};
    for (int which = 0; which < 3; ++which) {   // FEAT_IMAGE_UV: set, set, not set
        World w(1);
        image_world(w, which);
        dump_world(image_name[which], w);
    }
    // an instance over a TLAS subtree: no relative codes (rel_ok false), every code absolute, all
    // pad 0, stack16_ok from (n_prim_refs << 5) | 31: 1 with few slots; 0 at 1023 slots, where no
    // real code reaches 32767
    for (int n_blas : {12, 1023 - 62}) {
        World w(4);
        field_and_instance(w, 60, n_blas);
        dump_world(n_blas == 12 ? "instance_over_tlas_small" : "instance_over_tlas_1023", w, RT_ACCEL_SAH, true,
                   point_instance_at_tlas);
        if (n_blas != 12) dump_world("instance_beside_tlas_1023", w);   // the same tables unedited: relative codes
    }
    {   // one BVH instance's slot under two TLAS leaves: two slot visits, the sum (unedited: the max)
        World w(4);
        field_and_instance(w, 60, 12);
        dump_world("instance_slot_once", w);
        dump_world("instance_slot_twice", w, RT_ACCEL_SAH, true, reference_instance_twice);
    }
    // Stack16 needs <= 408 TLAS nodes and leaf codes below 32767: fields on both sides of each
    // bound (613 spheres make 406 nodes, 614 make 409; with leaves of up to 31 the TLAS stays
    // small and the codes decide: 1038 spheres fit, 1039 do not)
    for (int n : {300, 613, 614, 1100, 1038, 1039}) {
        World w(4);
        const bool big_leaves = n == 1038 || n == 1039;
        if (big_leaves) w.build.force_leaf = 16, w.build.max_leaf = 31;
        sphere_field(w, n);
        dump_world((std::string(big_leaves ? "sphere_field_leaf31_" : "sphere_field_") + std::to_string(n)).c_str(), w);
    }
    // the box invariant: negative radii and shutters inside / beside [0, 1] are lowered with the
    // product's own boxes; under an rt_world_bvh node they are refused at flatten in every mode;
    // built for the ray times [-1, 4] the shutter [2, 3] is still inside the range
    for (int accel = 0; accel < 3; ++accel) {
        World w(6), v(6);
        unbounded_by_reference(w, false);
        dump_world((std::string("unbounded_by_reference_") + accel_name[accel]).c_str(), w, accel);
        unbounded_by_reference(v, true);
        dump_world((std::string("unbounded_by_reference_under_bvh_") + accel_name[accel]).c_str(), v, accel);
    }
    {
        World w(6);
        w.build.time0 = -1.0;
        w.build.time1 = 4.0;
        unbounded_by_reference(w, false);
        dump_world("unbounded_by_reference_times_m1_4", w);
    }
    // n concentric spheres whose radii span 2^60: no centroid separates them, the SAH peels one
    // shell per level, and from recursion depth 20 on the builder's median split keeps the walk
    // within the kernel's 32 stack entries (concentric_200 reaches it, concentric_64 stops short)
    for (int n : {64, 200}) {
        World w(1);
        const int wh = white(w);
        for (int i = 0; i < n; ++i) w.push(w.sphere(wh, v3(0.0, 0.0, 0.0), std::ldexp(1.0, i % 60) * (1 + i / 60)));
        dump_world(("concentric_" + std::to_string(n)).c_str(), w);
    }
    // every SAH build option set alone (rt_world_set_build_option), on the final scene and the
    // Cornell smoke scene
    struct Option {
        const char* name;
        void (*set)(rtw::BuildOptions&);
    };
    static const Option options[6] = {
        {"c_isect_0p7", [](rtw::BuildOptions& b) { b.c_isect = 0.7; }},
        {"max_leaf_2", [](rtw::BuildOptions& b) { b.max_leaf = 2; }},   // 4 changes neither scene
        {"force_leaf_1", [](rtw::BuildOptions& b) { b.force_leaf = 1; }},
        {"root_leaf_0", [](rtw::BuildOptions& b) { b.root_leaf = 0; }},
        {"split_box_pairs_0", [](rtw::BuildOptions& b) { b.split_box_pairs = 0; }},
        {"split_blas_pairs_0", [](rtw::BuildOptions& b) { b.split_blas_pairs = 0; }},
    };
    for (int id : {7, 6})
        for (const Option& o : options) {
            World w(1);
            if (rtw::build_scene(w, id, gradient(), 4, 2)) return 1;
            o.set(w.build);
            dump_world(("scene" + std::to_string(id) + "_" + o.name).c_str(), w);
        }
    return 0;
}
