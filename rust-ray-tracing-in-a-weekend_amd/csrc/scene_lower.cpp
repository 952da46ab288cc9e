// scene_lower.cpp — validation of a (possibly foreign) rt_scene_soa and its lowering to what
// the kernels assume (scene_lower.hpp). Plain C++: no HIP, no context.
#include "scene_lower.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_map>

#include "rt/rt_abi.h"
#include "bvh_build.hpp"       // stack_need
#include "launch_shapes.hpp"   // kLdsNodeBytes
#include "scene_features.hpp"

namespace rtl {
namespace {

bool is_sphere(int k) { return k == RT_PRIM_SPHERE || k == RT_PRIM_MOVING_SPHERE; }
bool is_rect(int k) { return k == RT_PRIM_XY_RECT || k == RT_PRIM_XZ_RECT || k == RT_PRIM_YZ_RECT || k == RT_PRIM_BOX; }
bool is_simple(int k) { return k >= RT_PRIM_SPHERE && k <= RT_PRIM_BOX; }

// A leaf reference (child < 0): slots [first, first + count) of prim_refs.
struct Leaf {
    int first, count;
    int code() const { return (first << 5) | count; }
    int ref() const { return ~code(); }
};
Leaf leaf_of(int ref) { return Leaf{(~ref) >> 5, (~ref) & 31}; }

// Depth-first over what `ref` reaches in a checked, acyclic node graph: node(i) for a node,
// leaf(Leaf) for a leaf reference (ref itself may be one). With `seen`, a node marked there is
// skipped with everything below it and the nodes visited get marked; without, a node (and a
// leaf) reachable along two paths is visited twice.
template <class NodeFn, class LeafFn>
void walk(const rt_scene_soa& s, int ref, std::vector<uint8_t>* seen, NodeFn node, LeafFn leaf)
{
    std::vector<int> todo{ref};
    while (!todo.empty()) {
        const int r = todo.back();
        todo.pop_back();
        if (r < 0) {
            leaf(leaf_of(r));
            continue;
        }
        if (seen) {
            if ((*seen)[(size_t)r]) continue;
            (*seen)[(size_t)r] = 1;
        }
        node(r);
        todo.push_back(s.nodes[r].child[0]);
        todo.push_back(s.nodes[r].child[1]);
    }
}

// pre_leaf: a root child that is a leaf of <= 2 primitives whose box holds at least 8x the
// volume of its sibling's (a ground or fog sphere around the whole scene) is tested before the
// walk, which then starts at the sibling (in the kernel variants that do this). The closest hit
// does not depend on the order of the tests, so the image does not change
// (tests/test_gpu_parity.py); only SAH tables (the LINEAR / MEDIAN modes keep the reference's
// structures as they are).
void hoist_root_leaf(const rt_scene_soa& s, Lowered& L)
{
    if (s.accel != RT_ACCEL_SAH || s.tlas_root < 0 || s.tlas_root >= s.n_nodes) return;
    const rt_bvh_node& root = s.nodes[s.tlas_root];
    auto volume = [](const float* lo, const float* hi) {
        double v = 1.0;
        for (int a = 0; a < 3; ++a) v *= std::max(0.0, (double)hi[a] - (double)lo[a]);
        return v;
    };
    for (int c = 0; c < 2; ++c) {
        const int leaf = root.child[c], other = root.child[1 - c];
        if (leaf >= 0 || leaf_of(leaf).count > 2) continue;
        const float* lo = c ? root.lo1 : root.lo0;
        const float* hi = c ? root.hi1 : root.hi0;
        const double v = volume(lo, hi), vo = volume(c ? root.lo0 : root.lo1, c ? root.hi0 : root.hi1);
        if (!(v >= 8.0 * vo) || !std::isfinite(v)) continue;
        L.pre_leaf = leaf;
        std::copy(lo, lo + 3, L.pre_lo);
        std::copy(hi, hi + 3, L.pre_hi);
        L.pre_root = other;
        return;
    }
}

// What one instance's BVH root reaches.
struct Blas {
    std::vector<int> nodes;     // breadth-first, child 0 before child 1, each node once
    int base = 1 << 30;         // its smallest leaf slot
    int min_node = 1 << 30;     // its smallest node index
    bool rect = false, moving = false, imaged = false;   // holds a rect / box, a moving sphere, an image texture
    bool relative = false;      // its leaf codes have been made relative to base
};

}  // namespace

// Validates a (possibly foreign) SoA so the kernel never indexes out of bounds, never
// overruns its traversal stack and never walks a cycle; computes the stack needs itself
// (the tlas_depth / blas_depth fields are not trusted) and whether the TLAS really lies in
// nodes[0, n_tlas_nodes) (the kernel copies that prefix into LDS and then reads only LDS).
int validate(const rt_scene_soa& s, int& tlas_depth, int& blas_depth, int& n_tlas_nodes, std::string& err)
{
    auto fail = [&](int code, const char* msg) {
        err = msg;
        return code;
    };
    if (s.n_prim_refs >= (1 << 26) - 64) return fail(RT_ERR_UNSUPPORTED, "too many primitive references");
    if (s.n_prims < 0 || s.n_prim_refs < 0 || s.n_nodes < 0 || s.n_instances < 0 || s.n_materials < 0 ||
        s.n_textures < 0 || s.n_perlin < 0 || s.image_bytes < 0)
        return fail(RT_ERR_INVALID, "negative table size");
    if ((s.n_prims && !s.prims) || (s.n_prim_refs && !s.prim_refs) || (s.n_nodes && !s.nodes) ||
        (s.n_instances && !s.instances) || (s.n_materials && !s.materials) || (s.n_textures && !s.textures) ||
        (s.n_perlin && (!s.perlin_ranvec || !s.perlin_perm)) || (s.image_bytes && !s.image_data))
        return fail(RT_ERR_INVALID, "null table");
    for (int i = 0; i < s.n_prims; ++i) {
        const rt_prim& p = s.prims[i];
        if (p.kind < RT_PRIM_SPHERE || p.kind > RT_PRIM_MEDIUM) return fail(RT_ERR_INVALID, "bad prim kind");
        if (p.kind == RT_PRIM_INSTANCE && (p.a < 0 || p.a >= s.n_instances)) return fail(RT_ERR_INVALID, "bad instance");
        if (p.kind == RT_PRIM_MEDIUM) {
            if (p.a < 0 || p.a >= s.n_prims) return fail(RT_ERR_INVALID, "bad boundary");
            const int bk = s.prims[p.a].kind;  // boundary_t: a simple prim or an instance
            if (!is_simple(bk) && bk != RT_PRIM_INSTANCE) return fail(RT_ERR_UNSUPPORTED, "medium boundary kind");
        }
        if (p.kind != RT_PRIM_INSTANCE && (p.mat < 0 || p.mat >= s.n_materials)) return fail(RT_ERR_INVALID, "bad material");
    }
    for (int i = 0; i < s.n_materials; ++i) {
        const rt_material& m = s.materials[i];
        if (m.kind < RT_MAT_LAMBERTIAN || m.kind > RT_MAT_ISOTROPIC) return fail(RT_ERR_INVALID, "bad material kind");
        bool needs_tex = m.kind == RT_MAT_LAMBERTIAN || m.kind == RT_MAT_DIFFUSE_LIGHT || m.kind == RT_MAT_ISOTROPIC;
        if (needs_tex && (m.tex < 0 || m.tex >= s.n_textures)) return fail(RT_ERR_INVALID, "bad texture ref");
    }
    for (int i = 0; i < s.n_textures; ++i) {
        const rt_texture& t = s.textures[i];
        if (t.kind < RT_TEX_SOLID || t.kind > RT_TEX_IMAGE) return fail(RT_ERR_INVALID, "bad texture kind");
        if (t.kind == RT_TEX_NOISE && (t.perlin < 0 || t.perlin >= s.n_perlin)) return fail(RT_ERR_INVALID, "bad perlin");
        if (t.kind == RT_TEX_IMAGE && t.img_w > 0 &&
            (t.img_h <= 0 || t.img_offset < 0 || t.img_bps < 3 * (int64_t)t.img_w ||
             t.img_offset + t.img_bps * (int64_t)(t.img_h - 1) + 3 * (int64_t)t.img_w > s.image_bytes))
            return fail(RT_ERR_INVALID, "image texture out of range");
    }
    for (int i = 0; i < s.n_prim_refs; ++i)
        if (s.prim_refs[i] < 0 || s.prim_refs[i] >= s.n_prims) return fail(RT_ERR_INVALID, "bad prim ref");
    auto check_ref = [&](int ref) {
        if (ref >= 0) return ref < s.n_nodes;
        return leaf_of(ref).first + leaf_of(ref).count <= s.n_prim_refs;
    };
    for (int i = 0; i < s.n_nodes; ++i)
        if (!check_ref(s.nodes[i].child[0]) || !check_ref(s.nodes[i].child[1])) return fail(RT_ERR_INVALID, "bad node");
    if (!check_ref(s.tlas_root)) return fail(RT_ERR_INVALID, "bad tlas root");
    for (int i = 0; i < s.n_instances; ++i) {
        const rt_instance& in = s.instances[i];
        if (in.n_ops < 0 || in.n_ops > 4) return fail(RT_ERR_INVALID, "bad instance ops");
        if (in.child_kind != RT_CHILD_PRIM && in.child_kind != RT_CHILD_BVH) return fail(RT_ERR_INVALID, "bad instance child kind");
        if (in.child_kind == RT_CHILD_PRIM ? (in.child < 0 || in.child >= s.n_prims) : !check_ref(in.child))
            return fail(RT_ERR_INVALID, "bad instance child");
        if (in.child_kind == RT_CHILD_PRIM && !is_simple(s.prims[in.child].kind) &&
            s.prims[in.child].kind != RT_PRIM_MEDIUM)
            return fail(RT_ERR_UNSUPPORTED, "instance child must be a primitive, a medium or a BVH");
    }
    // what the kernel's nested calls assume (flatten.cpp lowers any nesting into this shape):
    // a medium's boundary instance has no medium child (no recursion), and an instance BLAS
    // holds simple primitives only
    for (int i = 0; i < s.n_prims; ++i) {
        const rt_prim& p = s.prims[i];
        if (p.kind != RT_PRIM_MEDIUM || s.prims[p.a].kind != RT_PRIM_INSTANCE) continue;
        const rt_instance& in = s.instances[s.prims[p.a].a];
        if (in.child_kind == RT_CHILD_PRIM && s.prims[in.child].kind == RT_PRIM_MEDIUM)
            return fail(RT_ERR_UNSUPPORTED, "a medium's boundary holds a medium");
    }
    // stack needs (the kernel: TLAS walk in entries [0, tlas), a nested BLAS walk above it), by
    // the rule flatten.cpp builds with (rtb::stack_need), recomputed here from the tables alone;
    // a cycle is found instead of walked forever (the persistent kernel would spin on it)
    rtb::StackMemo memo;
    memo.resize((size_t)s.n_nodes);
    const int t = rtb::stack_need(s.nodes, s.tlas_root, memo);
    if (t < 0) return fail(RT_ERR_INVALID, "cycle in the TLAS node graph");
    tlas_depth = t + 1;  // + 1 as flatten.cpp records it
    blas_depth = 0;
    // The walks of instance BLASes share the memo: a BLAS shared by many instances, or a
    // subtree of one already walked, costs nothing the second time (O(nodes) in total, not
    // O(instances x nodes)). Likewise `checked` marks subtrees whose leaves were already found
    // to hold simple primitives.
    std::vector<uint8_t> checked((size_t)s.n_nodes, 0);
    bool simple = true;
    for (int i = 0; i < s.n_instances && simple; ++i) {
        const rt_instance& in = s.instances[i];
        if (in.child_kind != RT_CHILD_BVH) continue;
        const int b = rtb::stack_need(s.nodes, in.child, memo);
        if (b < 0) return fail(RT_ERR_INVALID, "cycle in an instance BVH");
        blas_depth = std::max(blas_depth, b + 1);
        walk(s, in.child, &checked, [](int) {}, [&](Leaf l) {
            for (int j = l.first; j < l.first + l.count; ++j) simple = simple && is_simple(s.prims[s.prim_refs[j]].kind);
        });
    }
    if (!simple) return fail(RT_ERR_UNSUPPORTED, "an instance BVH holds a non-primitive");
    if (tlas_depth > 32 || blas_depth > 32) return fail(RT_ERR_UNSUPPORTED, "BVH too deep for the traversal stack");
    // the TLAS-in-LDS claim: every node reachable from the root lies in [0, n_tlas_nodes)
    n_tlas_nodes = 0;
    if (s.n_tlas_nodes > 0 && s.n_tlas_nodes <= s.n_nodes && s.tlas_root == 0) {
        bool inside = true;
        std::vector<uint8_t> seen((size_t)s.n_nodes, 0);
        walk(s, 0, &seen,[&](int i) { inside = inside && i < s.n_tlas_nodes; }, [](Leaf) {});
        if (inside) n_tlas_nodes = s.n_tlas_nodes;
    }
    return RT_OK;
}

int lower(const rt_scene_soa& s, bool hoist, Lowered& L, std::string& err)
{
    L = Lowered{};
    const int rc = validate(s, L.tlas_depth, L.blas_depth, L.n_tlas_nodes, err);
    if (rc) return rc;
    uint32_t feat = 0;

    // The device's primitive records. A Sphere is stored as a MovingSphere that does not
    // move (velocity 0, a = 1: the centre c0 + 0 * time is c0 bit for bit), so the kernel's
    // sphere test reads no kind and selects nothing (sphere_center). A MovingSphere's a says
    // whether its shutter is [0, 1] ((time - 0) / (1 - 0) is time exactly); it is recomputed
    // here rather than trusted from a foreign SoA. Only a scene with another shutter needs
    // FEAT_SHUTTER (the per-primitive flag and the division); without it a sphere test issues
    // all its loads at once. Then the records in leaf-slot order (prims[prim_refs[j]]): the leaf
    // loops read a record without first loading its index.
    L.prims.assign(s.prims, s.prims + s.n_prims);
    for (rt_prim& p : L.prims) {
        if (p.kind == RT_PRIM_SPHERE) {
            p.a = 1;
            p.p[5] = p.p[6] = p.p[7] = p.p[8] = 0.0;
            p.p[9] = 1.0;
        } else if (p.kind == RT_PRIM_MOVING_SPHERE) {
            p.a = (p.p[8] == 0.0 && p.p[9] == 1.0) ? 1 : 0;
            if (!p.a) feat |= rtk::FEAT_SHUTTER;
        } else if (p.kind == RT_PRIM_INSTANCE) {
            // b = 1: the instance's child is a BVH (the kernel defers the first such walk of a
            // cast, RT_DEFER_INST); a single child primitive is tested where the walk meets it
            p.b = s.instances[p.a].child_kind == RT_CHILD_BVH ? 1 : 0;
        }
    }
    L.leaf_prims.resize((size_t)s.n_prim_refs);
    for (int j = 0; j < s.n_prim_refs; ++j) L.leaf_prims[(size_t)j] = L.prims[(size_t)s.prim_refs[j]];

    // a sphere that really moves (nonzero velocity, or a shutter other than [0, 1], whose
    // centre may not be c0); an image-textured primitive
    auto moving = [&](int i) {
        const rt_prim& q = L.prims[(size_t)i];
        return q.kind == RT_PRIM_MOVING_SPHERE && (!q.a || q.p[5] != 0.0 || q.p[6] != 0.0 || q.p[7] != 0.0);
    };
    auto imaged = [&](int i) {
        const rt_prim& p = s.prims[i];
        if (p.kind == RT_PRIM_INSTANCE || p.kind == RT_PRIM_MEDIUM) return false;
        const rt_material& m = s.materials[p.mat];
        return m.kind != RT_MAT_METAL && m.kind != RT_MAT_DIELECTRIC && s.textures[m.tex].kind == RT_TEX_IMAGE;
    };

    // Every distinct instance-BVH root, scanned once however many instances share it.
    std::unordered_map<int, Blas> blases;
    std::vector<uint8_t> seen((size_t)s.n_nodes, 0);
    for (int ii = 0; ii < s.n_instances; ++ii) {
        const rt_instance& in = s.instances[ii];
        if (in.child_kind != RT_CHILD_BVH || blases.count(in.child)) continue;
        Blas& b = blases[in.child];
        auto leaf = [&](Leaf l) {
            b.base = std::min(b.base, l.first);
            for (int j = l.first; j < l.first + l.count; ++j) {
                const int p = s.prim_refs[j];
                b.rect = b.rect || is_rect(s.prims[p].kind);
                b.moving = b.moving || moving(p);
                b.imaged = b.imaged || imaged(p);
            }
        };
        auto reach = [&](int ref) {
            if (ref < 0) return leaf(leaf_of(ref));
            if (seen[(size_t)ref]) return;
            seen[(size_t)ref] = 1;
            b.min_node = std::min(b.min_node, ref);
            b.nodes.push_back(ref);
        };
        reach(in.child);
        for (size_t k = 0; k < b.nodes.size(); ++k) {
            const int i = b.nodes[k];   // (reach grows b.nodes)
            reach(s.nodes[i].child[0]);
            reach(s.nodes[i].child[1]);
        }
        for (int i : b.nodes) seen[(size_t)i] = 0;
    }

    // Device copies of the nodes and instances in which every instance BLAS's leaf codes count
    // slots from that BLAS's first leaf slot (kept in the device rt_instance.pad): the codes of
    // both walks then stay small enough for 16-bit stack entries (Stack16: a 1000-sphere BLAS at
    // slots 410..1409 has relative slots 0..999). Only when every BLAS is disjoint from the TLAS
    // and from the other BLASes (or shares nodes with one of the same base); otherwise every
    // code of the scene stays absolute and it takes the 32-bit stack (stack16_ok 0).
    L.nodes.assign(s.nodes, s.nodes + s.n_nodes);
    L.instances.assign(s.instances, s.instances + s.n_instances);
    for (rt_instance& in : L.instances) in.pad = 0;
    int max_code = 0;   // the largest leaf code ((first slot << 5) | count) either walk pushes
    {
        std::vector<uint8_t> in_tlas((size_t)s.n_nodes, 0);
        walk(s, s.tlas_root, &in_tlas, [](int) {}, [&](Leaf l) { max_code = std::max(max_code, l.code()); });
        std::vector<int> owner((size_t)s.n_nodes, -1);   // the base of the BLAS a node was rewritten for
        auto rel = [&](int ref, int base) {
            const Leaf l{leaf_of(ref).first - base, leaf_of(ref).count};
            max_code = std::max(max_code, l.code());
            return l.ref();
        };
        bool rel_ok = true;
        for (rt_instance& in : L.instances) {
            if (in.child_kind != RT_CHILD_BVH) continue;
            Blas& b = blases.at(in.child);
            if (!b.relative) {
                for (int i : b.nodes)
                    if (in_tlas[(size_t)i] || (owner[(size_t)i] >= 0 && owner[(size_t)i] != b.base)) rel_ok = false;
                if (!rel_ok) break;
                for (int i : b.nodes) {
                    if (owner[(size_t)i] == b.base) continue;   // shared with a BLAS already rewritten
                    owner[(size_t)i] = b.base;
                    for (int& ch : L.nodes[(size_t)i].child)
                        if (ch < 0) ch = rel(ch, b.base);
                }
                b.relative = true;
            }
            if (in.child < 0) in.child = rel(in.child, b.base);
            in.pad = b.base;
        }
        if (!rel_ok) {   // absolute codes everywhere
            L.nodes.assign(s.nodes, s.nodes + s.n_nodes);
            L.instances.assign(s.instances, s.instances + s.n_instances);
            for (rt_instance& in : L.instances) in.pad = 0;
            max_code = (s.n_prim_refs << 5) | 31;
        }
    }

    // The largest instance BLAS in BFS order right after the TLAS prefix (device node order
    // only): a launch stages its top levels in LDS (SceneDev.n_lds_blas), where the nested
    // walk reads them instead of waiting on L2 for every level. Needs the TLAS prefix and a
    // BLAS disjoint from it (validate's n_tlas_nodes); otherwise nothing is staged.
    const Blas* best = nullptr;
    for (const rt_instance& in : L.instances) {   // the first of the largest, in instance order
        if (in.child_kind != RT_CHILD_BVH || in.child < L.n_tlas_nodes) continue;
        const Blas& b = blases.at(in.child);
        if (b.min_node >= L.n_tlas_nodes && b.nodes.size() > (best ? best->nodes.size() : 0)) best = &b;
    }
    if (best && (L.n_tlas_nodes > 0 || s.tlas_root < 0)) {
        std::vector<int> perm((size_t)s.n_nodes, -1);
        int next = 0;
        while (next < L.n_tlas_nodes) perm[(size_t)next] = next, ++next;
        for (int b : best->nodes) perm[(size_t)b] = next++;
        for (int& p : perm)
            if (p < 0) p = next++;
        std::vector<rt_bvh_node> moved((size_t)s.n_nodes);
        for (int i = 0; i < s.n_nodes; ++i) {
            rt_bvh_node nd = L.nodes[(size_t)i];
            for (int& ch : nd.child)
                if (ch >= 0) ch = perm[(size_t)ch];
            moved[(size_t)perm[(size_t)i]] = nd;
        }
        L.nodes.swap(moved);
        for (rt_instance& in : L.instances)
            if (in.child_kind == RT_CHILD_BVH && in.child >= 0) in.child = perm[(size_t)in.child];
        L.n_blas_bfs = (int)best->nodes.size();
    }

    if (hoist) hoist_root_leaf(s, L);
    // Stack16 (trace_types.hpp): node records (kLdsNodeBytes each) at LDS addresses < 32 KB, BLAS node
    // indices < 32768, and leaf codes ((first slot << 5) | count, stored complemented; BLAS slots
    // relative, above) strictly above the -32768 = ~32767 sentinel: every code < 32767 (a leaf
    // at first slot 1023 holding 31 primitives would complement to the sentinel itself)
    L.stack16_ok = (L.n_tlas_nodes * (int64_t)rtk::kLdsNodeBytes <= 32767 - (int64_t)rtk::kLdsNodeBytes && max_code < 32767 && s.n_nodes <= 32767) ? 1 : 0;
    // traversal stack: TLAS walk, then a nested BLAS walk (instances) above it, sized from the
    // depths validate measured (<= 32 each), each walk's bottom entry holding its RT_DONE
    // sentinel (traverse): the 66-entry scratch stack always fits
    L.blas_base = L.tlas_depth + 1;
    L.stack_entries = L.tlas_depth + 1 + (L.blas_depth > 0 ? L.blas_depth + 1 : 0);
    // A BLAS walk nests in the top-level walk only for a cast's second instance over a BVH (the
    // first is deferred until the top-level walk ends, then walks from entry 0: RT_DEFER_INST),
    // an instance over a medium, or a medium whose boundary is an instance. A scene whose top
    // level holds one instance over a BVH and none of the others (the final scene) needs the
    // larger of the two walks, not their sum: 13 entries instead of 26 per lane, 12 KB less LDS
    // per block. Counted per slot visit, not per primitive: a cast can meet a slot that two
    // leaves hold twice, and only the first meeting is deferred.
    if (RT_DEFER_INST && L.blas_depth > 0) {
        int n_inst = 0;
        bool inst_boundary = false;
        walk(s, s.tlas_root, nullptr, [](int) {}, [&](Leaf l) {
            for (int j = l.first; j < l.first + l.count; ++j) {
                const rt_prim& p = s.prims[s.prim_refs[j]];
                if (p.kind == RT_PRIM_INSTANCE) {   // an instance that may walk a BLAS
                    const rt_instance& in = s.instances[p.a];
                    if (in.child_kind == RT_CHILD_BVH) ++n_inst;
                    else if (s.prims[in.child].kind == RT_PRIM_MEDIUM) inst_boundary = true;   // never deferred
                }
                if (p.kind == RT_PRIM_MEDIUM && s.prims[p.a].kind == RT_PRIM_INSTANCE) inst_boundary = true;
            }
        });
        if (n_inst <= 1 && !inst_boundary) L.stack_entries = std::max(L.tlas_depth + 1, L.blas_depth + 1);
    }

    // The features (the kernel variant drops the code of the others). What instances and medium
    // boundaries reach counts separately: rects / boxes under an instance (FEAT_INST_RECT),
    // medium boundaries other than spheres (FEAT_MEDIUM_INST), and a really moving sphere under
    // an instance or as a medium's boundary (FEAT_NEST_MOVING; without it the kernel tests the
    // spheres there as static, FEAT_STATIC: c0, no velocity loads). FEAT_IMAGE_UV: an
    // image-textured primitive whose hit record must carry its uv inputs (a rect or box, or
    // anything under an instance); otherwise uv comes from a top-level sphere's normal.
    bool image_uv = false;
    for (int i = 0; i < s.n_prims; ++i) {
        const rt_prim& p = s.prims[i];
        if (is_sphere(p.kind)) L.has_spheres = 1;
        if (is_rect(p.kind)) feat |= rtk::FEAT_RECT;
        if (p.kind == RT_PRIM_INSTANCE) feat |= rtk::FEAT_INST;
        if (p.kind == RT_PRIM_MEDIUM) {
            feat |= rtk::FEAT_MEDIUM;
            if (!is_sphere(s.prims[p.a].kind)) feat |= rtk::FEAT_MEDIUM_INST;
            if (moving(p.a)) feat |= rtk::FEAT_NEST_MOVING;
        }
        if (!is_sphere(p.kind) && imaged(i)) image_uv = true;
    }
    for (int ii = 0; ii < s.n_instances; ++ii) {
        const rt_instance& in = s.instances[ii];
        if (in.child_kind == RT_CHILD_BVH) {
            const Blas& b = blases.at(in.child);
            feat |= rtk::FEAT_INST_BLAS | (b.rect ? rtk::FEAT_INST_RECT : 0) | (b.moving ? rtk::FEAT_NEST_MOVING : 0);
            image_uv = image_uv || b.imaged;
            continue;
        }
        // one primitive; a medium's own boundary is covered by the loop over the primitives
        const int ck = s.prims[in.child].kind;
        if (is_rect(ck)) feat |= rtk::FEAT_INST_RECT;
        if (ck == RT_PRIM_MEDIUM) feat |= rtk::FEAT_INST_MEDIUM;
        if (moving(in.child)) feat |= rtk::FEAT_NEST_MOVING;
        image_uv = image_uv || imaged(in.child);
    }
    for (int i = 0; i < s.n_textures; ++i) {
        if (s.textures[i].kind == RT_TEX_NOISE) feat |= rtk::FEAT_NOISE;
        if (s.textures[i].kind == RT_TEX_IMAGE) feat |= rtk::FEAT_IMAGE;
    }
    if (image_uv) feat |= rtk::FEAT_IMAGE_UV;
    L.features = feat;
    // any DiffuseLight: without one, a hit never emits (shade_begin skips its material read)
    for (int i = 0; i < s.n_materials; ++i)
        if (s.materials[i].kind == RT_MAT_DIFFUSE_LIGHT) L.has_lights = 1;
    L.pad_extent = s.pad_extent > 0.0 && std::isfinite(s.pad_extent) ? s.pad_extent : 0.0;
    for (int i = 0; i < s.n_prims; ++i)
        if (s.prims[i].kind == RT_PRIM_MOVING_SPHERE) L.has_moving = 1;
    L.time_lo = s.time_lo;
    L.time_hi = s.time_hi;
    return RT_OK;
}

}  // namespace rtl
