// flatten.cpp — lowers the World's Hittable tree into the SoA tables of rt_scene.h: primitives,
// instances and media, each with the box its hit test stays inside; bvh_build.cpp builds the
// hierarchies the megakernel traverses over those boxes.
//
// Lowering rules (hittable.rs:30-41):
//   Sphere / MovingSphere / XY,XZ,YZ rects / Box   -> one rt_prim each
//   BvhNode (reference median BVH, :77-130)        -> dissolved; its leaves join the
//                                                     enclosing SAH BVH (closest-hit is
//                                                     independent of the hierarchy, see
//                                                     the box invariant below)
//   Translate / RotateY chains (:232-244, :386-415) -> rt_instance (<= 4 ops) whose child
//                                                     is a single prim or its own BLAS
//   ConstantMedium (:417-473)                       -> RT_PRIM_MEDIUM whose boundary is a
//                                                     hidden prim (sphere / box / instance)
// The top-level list becomes the TLAS. Nested instances, BVHs and media are lowered by
// pushing Translate/RotateY chains down (lower_instance); a medium boundary that holds
// instances or media, and chains longer than 4 ops, are not (RT_ERR_UNSUPPORTED).
//
// accel (rt_scene.h) picks the hierarchy (bvh_build.hpp): SAH (above), LINEAR (every list a
// chain of unbounded nodes over <=31-prim leaves, in list order: hit_hittables' linear scan), or
// MEDIAN (the reference's BvhNodes kept node for node by lower_ref_bvh, the top-level list a chain).
//
// The box invariant. "Closest hit is independent of the hierarchy" holds only while every node
// box bounds everything the primitive tests below it can accept. The reference's own
// bounding_box does not give that (a radius < 0 inverts a sphere's box; a moving sphere's box
// spans its own shutter, while its centre extrapolates to any ray time), so every box here
// comes from Lowering::bound_of: |r|, and a moving sphere's centres over the ray times
// [time_lo, time_hi] the tables are built for — [0, 1] unless RT_BUILD_TIME0 / _TIME1 say
// otherwise, recorded in rt_scene_soa; a render whose camera shutter leaves that range is
// refused (launch_plan.cpp) when the scene holds a moving sphere. The one place the reference
// culls by its own boxes is a BvhNode (rt_world_bvh): a node with a child whose reference box
// does not bound it is refused at flatten (RT_ERR_UNSUPPORTED, check_ref_bvhs), in every accel
// mode, because the reference's image then depends on its hierarchy.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "rt/rt_abi.h"
#include "bvh_build.hpp"
#include "scene_model.hpp"

namespace rtw {

namespace {

using rtb::Item;

struct Lowering {
    World& w;
    FlatScene& f;
    std::string& err;
    const int accel;
    const rtb::SahParams sah;
    const double time_lo, time_hi;   // the ray times the boxes hold for
    double world_extent = 0.0;       // M: max |coordinate| over the top-level boxes (measure_extent)
    int blas_depth = 0;              // max over instance BLASes
    rtb::StackMemo memo{};           // of the stack needs, shared by every BLAS and the TLAS

    int add_prim(const rt_prim& p)
    {
        f.prims.push_back(p);
        return (int)f.prims.size() - 1;
    }

    static rt_prim blank(int kind, int mat)
    {
        rt_prim p;
        std::memset(&p, 0, sizeof p);
        p.kind = kind;
        p.mat = mat;
        return p;
    }

    bool is_simple(HKind k) const
    {
        return k == HKind::Sphere || k == HKind::MovingSphere || k == HKind::XYRect || k == HKind::XZRect ||
               k == HKind::YZRect || k == HKind::Box;
    }

    // pad_abs: the f32 box padding of the space the primitive is lowered in (pad_through)
    int lower_simple(int id, double pad_abs)
    {
        const HNode& h = w.nodes[id];
        rt_prim p = blank(0, h.mat - 1);
        switch (h.kind) {
        case HKind::Sphere:
            p.kind = RT_PRIM_SPHERE;
            p.p[0] = h.c0.x; p.p[1] = h.c0.y; p.p[2] = h.c0.z;
            p.p[3] = h.radius;
            p.p[4] = 1.0 / h.radius;  // the reference's Div: (1/r) * v (math.rs:260-266)
            break;
        case HKind::MovingSphere:
            p.kind = RT_PRIM_MOVING_SPHERE;
            p.p[0] = h.c0.x; p.p[1] = h.c0.y; p.p[2] = h.c0.z;
            p.p[3] = h.radius;
            p.p[4] = 1.0 / h.radius;
            p.p[5] = h.c1.x - h.c0.x; p.p[6] = h.c1.y - h.c0.y; p.p[7] = h.c1.z - h.c0.z;  // hittable.rs:557
            p.p[8] = h.t0; p.p[9] = h.t1;
            p.a = (h.t0 == 0.0 && h.t1 == 1.0) ? 1 : 0;  // (time - 0) / (1 - 0) == time exactly
            break;
        case HKind::XYRect: case HKind::XZRect: case HKind::YZRect:
            p.kind = h.kind == HKind::XYRect ? RT_PRIM_XY_RECT : h.kind == HKind::XZRect ? RT_PRIM_XZ_RECT
                                                                                         : RT_PRIM_YZ_RECT;
            p.p[0] = h.a0; p.p[1] = h.a1; p.p[2] = h.b0; p.p[3] = h.b1; p.p[4] = h.k;
            break;
        case HKind::Box: {
            p.kind = RT_PRIM_BOX;
            p.p[0] = h.bmin.x; p.p[1] = h.bmin.y; p.p[2] = h.bmin.z;
            p.p[3] = h.bmax.x; p.p[4] = h.bmax.y; p.p[5] = h.bmax.z;
            // the box's own bounds in f32, padded and rounded outward like a BVH node's
            // (rt_scene.h; the kernel's per-box pre-test measured slower and is not built)
            const double lo[3] = {h.bmin.x, h.bmin.y, h.bmin.z}, hi[3] = {h.bmax.x, h.bmax.y, h.bmax.z};
            float fb[6];
            rtb::to_f32_box(lo, hi, pad_abs, fb, fb + 3);
            std::memcpy(&p.p[6], fb, sizeof fb);
            p.b = 1;
            break;
        }
        default: break;
        }
        return add_prim(p);
    }

    // ---- the box invariant ---------------------------------------------------------------
    // Every box the kernel walks bounds what the hit tests below it accept, for every ray time in
    // [time_lo, time_hi]. World::bounding_box (the reference's, hittable.rs:475-554) does not:
    // a sphere of radius r < 0 (hit by its |r|, hittable.rs:254-288) gets the inverted box
    // c - r .. c + r, and a moving sphere the hull of its centres at its own shutter t0, t1 while
    // MovingSphere::center extrapolates to any ray time (:556-558). The reference's top-level list
    // is a linear scan and never notices; here the list is a BVH. So the boxes are the product's
    // own: |r|, and the centres at the two ends of the time range (the centre is linear in time).
    // For r > 0 and a shutter equal to the range they are the reference's, bit for bit.
    static AABB hull(const AABB& a, const AABB& b)
    {
        return AABB{v3(std::fmin(a.minimum.x, b.minimum.x), std::fmin(a.minimum.y, b.minimum.y),
                       std::fmin(a.minimum.z, b.minimum.z)),
                    v3(std::fmax(a.maximum.x, b.maximum.x), std::fmax(a.maximum.y, b.maximum.y),
                       std::fmax(a.maximum.z, b.maximum.z))};
    }

    AABB bound_of(int hid) const
    {
        const HNode& h = w.nodes[hid];
        switch (h.kind) {
        case HKind::Sphere: {
            const double r = std::fabs(h.radius);
            return AABB{h.c0 - v3(r, r, r), h.c0 + v3(r, r, r)};
        }
        case HKind::MovingSphere: {
            const double r = std::fabs(h.radius);
            const V3 a = h.c0 + (h.c1 - h.c0) * ((time_lo - h.t0) / (h.t1 - h.t0));   // hittable.rs:556-558
            const V3 b = h.c0 + (h.c1 - h.c0) * ((time_hi - h.t0) / (h.t1 - h.t0));
            return hull(AABB{a - v3(r, r, r), a + v3(r, r, r)}, AABB{b - v3(r, r, r), b + v3(r, r, r)});
        }
        case HKind::BvhNode: return h.right == h.left ? bound_of(h.left) : hull(bound_of(h.left), bound_of(h.right));
        case HKind::Translate: {
            const AABB b = bound_of(h.ptr);
            return AABB{b.minimum + h.offset, b.maximum + h.offset};
        }
        case HKind::RotateY: {   // the eight corners, as hittable.rs:147-199 rotates the child's box
            const AABB b = bound_of(h.ptr);
            AABB r{v3(INFINITY, INFINITY, INFINITY), v3(-INFINITY, -INFINITY, -INFINITY)};
            for (int k = 0; k < 8; ++k) {
                const double x = (k & 4) ? b.maximum.x : b.minimum.x, y = (k & 2) ? b.maximum.y : b.minimum.y;
                const double z = (k & 1) ? b.maximum.z : b.minimum.z;
                const double nx = h.cos_theta * x + h.sin_theta * z, nz = -h.sin_theta * x + h.cos_theta * z;
                r = hull(r, AABB{v3(nx, y, nz), v3(nx, y, nz)});
            }
            return r;
        }
        case HKind::ConstantMedium: return bound_of(h.ptr);
        default: {   // rects and boxes: the reference's box bounds them
            AABB b;
            w.bounding_box(hid, 0.0, 1.0, b);
            return b;
        }
        }
    }

    static const char* kind_name(HKind k)
    {
        switch (k) {
        case HKind::Sphere: return "sphere";
        case HKind::MovingSphere: return "moving sphere";
        case HKind::BvhNode: return "bvh node";
        case HKind::XYRect: case HKind::XZRect: case HKind::YZRect: return "rect";
        case HKind::Box: return "box";
        case HKind::Translate: return "translate";
        case HKind::RotateY: return "rotate_y";
        case HKind::ConstantMedium: return "constant medium";
        }
        return "hittable";
    }

    // Under an rt_world_bvh node the reference itself culls by its own boxes (hittable.rs:290-306,
    // aabb.rs:77-103: an inverted box is never hit), so where such a box does not bound its child the
    // reference's image depends on its hierarchy, which neither a SAH BVH nor a list scan
    // reproduces. Such a node is refused: every child's reference box must contain the child's bound.
    int check_ref_bvhs()
    {
        std::vector<char> seen(w.nodes.size(), 0);
        std::vector<int> todo(w.hittables.begin(), w.hittables.end());
        bool nested = false;
        while (!todo.empty()) {
            const int id = todo.back();
            todo.pop_back();
            if (!w.valid_hittable(id) || seen[(size_t)id]) continue;
            seen[(size_t)id] = 1;
            const HNode& h = w.nodes[id];
            if (h.kind == HKind::Translate || h.kind == HKind::RotateY || h.kind == HKind::ConstantMedium) todo.push_back(h.ptr);
            if (h.kind != HKind::BvhNode) continue;
            for (int c : {h.left, h.right}) {
                todo.push_back(c);
                if (!w.valid_hittable(c)) continue;
                AABB ref;
                const AABB own = bound_of(c);
                const bool ok = w.bounding_box(c, 0.0, 1.0, ref) &&
                                ref.minimum.x <= own.minimum.x && ref.minimum.y <= own.minimum.y && ref.minimum.z <= own.minimum.z &&
                                ref.maximum.x >= own.maximum.x && ref.maximum.y >= own.maximum.y && ref.maximum.z >= own.maximum.z;
                // (a child that is a BvhNode itself fails only through a child of its own, named when
                // the walk reaches it: its reference box is the hull of its children's)
                if (!ok && w.nodes[c].kind == HKind::BvhNode) {
                    nested = true;
                    continue;
                }
                if (!ok) {
                    err = "rt_world_bvh node " + std::to_string(id) + ": the reference's box of its child " + std::to_string(c) +
                          " (a " + kind_name(w.nodes[c].kind) + ") does not bound what that child's hit test accepts for ray times in [" +
                          std::to_string(time_lo) + ", " + std::to_string(time_hi) +
                          "] (a negative radius, or a moving sphere's shutter inside that range); the reference culls by that box";
                    return RT_ERR_UNSUPPORTED;
                }
            }
        }
        if (nested) {   // not reached while a BvhNode's box is the hull of its children's
            err = "an rt_world_bvh node's reference box does not bound its children";
            return RT_ERR_UNSUPPORTED;
        }
        return RT_OK;
    }

    // M for the f32-slab padding (rtb::to_f32_box), before anything is lowered: instances build
    // their BLAS while being lowered
    void measure_extent()
    {
        for (int id : w.hittables) {
            if (!w.valid_hittable(id)) continue;
            const AABB b = bound_of(id);
            const double c[6] = {b.minimum.x, b.minimum.y, b.minimum.z, b.maximum.x, b.maximum.y, b.maximum.z};
            for (double v : c)
                if (std::isfinite(v)) world_extent = std::max(world_extent, std::fabs(v));
        }
    }

    // costly (rtb::Item): a Box, a medium, or an instance over a BVH
    static Item item_box(int id, const AABB& b, bool costly, bool subtree = false)
    {
        const double lo[3] = {b.minimum.x, b.minimum.y, b.minimum.z}, hi[3] = {b.maximum.x, b.maximum.y, b.maximum.z};
        return Item(id, lo, hi, costly, subtree);
    }
    Item item_of(int prim, int hid, bool costly) const { return item_box(prim, bound_of(hid), costly); }
    Item simple_item(int hid, double pad_abs) { return item_of(lower_simple(hid, pad_abs), hid, w.nodes[hid].kind == HKind::Box); }

    // ---- Translate / RotateY (hittable.rs:232-244, 386-415) and general nesting --------
    // A chain of ops (outermost first) is pushed down through everything under it: for the
    // closest hit, Outer(BVH[a, b]) = BVH[Outer(a), Outer(b)] (the ray is transformed the
    // same way for each child, the hit parameter t is the ray's, and the record is mapped
    // back op by op — with each op's set_face_normal quirk — for the winning child only),
    // and Outer(Inner(x)) is one chain of Outer's ops followed by Inner's. So any nesting of
    // instances, BVHs and media lowers to instances whose child is one primitive, one medium
    // or a BLAS of primitives, each with a chain of <= 4 ops.
    struct Ops {
        int n = 0;
        int32_t kind[4] = {0, 0, 0, 0};
        double op[4][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    };

    // Appends the Translate / RotateY chain starting at id to ops; returns the node it ends on.
    int chain(int id, Ops& ops, int& rc)
    {
        int cur = id;
        while (w.nodes[cur].kind == HKind::Translate || w.nodes[cur].kind == HKind::RotateY) {
            if (ops.n == 4) {
                err = "instance chain longer than 4 Translate/RotateY ops";
                rc = RT_ERR_UNSUPPORTED;
                return -1;
            }
            const HNode& h = w.nodes[cur];
            if (h.kind == HKind::Translate) {
                ops.kind[ops.n] = RT_OP_TRANSLATE;
                ops.op[ops.n][0] = h.offset.x; ops.op[ops.n][1] = h.offset.y; ops.op[ops.n][2] = h.offset.z;
            } else {
                ops.kind[ops.n] = RT_OP_ROTATE_Y;
                ops.op[ops.n][0] = h.sin_theta; ops.op[ops.n][1] = h.cos_theta; ops.op[ops.n][2] = 0.0;
            }
            ops.n++;
            cur = h.ptr;
        }
        return cur;
    }

    // The world box of an object-space box seen through ops (corners mapped back op by op,
    // innermost first: rotate back x' = c x + s z, z' = -s x + c z; translate back + offset).
    static AABB box_through(const Ops& ops, AABB b)
    {
        for (int i = ops.n - 1; i >= 0; --i) {
            if (ops.kind[i] == RT_OP_TRANSLATE) {
                const V3 off = v3(ops.op[i][0], ops.op[i][1], ops.op[i][2]);
                b.minimum = b.minimum + off;
                b.maximum = b.maximum + off;
                continue;
            }
            const double sn = ops.op[i][0], cs = ops.op[i][1];
            AABB r{v3(INFINITY, b.minimum.y, INFINITY), v3(-INFINITY, b.maximum.y, -INFINITY)};
            for (int k = 0; k < 4; ++k) {
                const double x = (k & 1) ? b.maximum.x : b.minimum.x, z = (k & 2) ? b.maximum.z : b.minimum.z;
                const double nx = cs * x + sn * z, nz = -sn * x + cs * z;
                r.minimum.x = std::min(r.minimum.x, nx); r.maximum.x = std::max(r.maximum.x, nx);
                r.minimum.z = std::min(r.minimum.z, nz); r.maximum.z = std::max(r.maximum.z, nz);
            }
            b = r;
        }
        return b;
    }

    int make_instance(const Ops& ops, int child_kind, int child)
    {
        rt_instance in;
        std::memset(&in, 0, sizeof in);
        in.n_ops = ops.n;
        in.child_kind = child_kind;
        in.child = child;
        for (int i = 0; i < ops.n; ++i) {
            in.op_kind[i] = ops.kind[i];
            for (int a = 0; a < 3; ++a) in.op[i][a] = ops.op[i][a];
        }
        f.instances.push_back(in);
        rt_prim p = blank(RT_PRIM_INSTANCE, -1);
        p.a = (int)f.instances.size() - 1;
        return add_prim(p);
    }

    // Box padding (rtb::to_f32_box's pad_abs) for object space seen through ops: object-space
    // origins have |o_obj| <= |o_world| + sum |offsets|, which the padding must cover. No ops:
    // world space.
    double pad_through(const Ops& ops) const
    {
        double off = 0.0;
        for (int i = 0; i < ops.n; ++i)
            if (ops.kind[i] == RT_OP_TRANSLATE)
                off += std::sqrt(ops.op[i][0] * ops.op[i][0] + ops.op[i][1] * ops.op[i][1] + ops.op[i][2] * ops.op[i][2]);
        return 0x1.0p-18 * (world_extent + off);
    }

    int build_bvh(std::vector<Item>& items, double pad_abs, bool in_blas)
    {
        if (accel != RT_ACCEL_SAH) return rtb::build_chain(items, f.nodes, f.prim_refs);
        return rtb::build_sah(items, sah, pad_abs, in_blas, f.nodes, f.prim_refs);
    }

    // + 1 as rt_scene_soa records its depths
    int depth_of(int root)
    {
        memo.resize(f.nodes.size());
        return rtb::stack_need(f.nodes.data(), root, memo) + 1;
    }

    // A BLAS over simple leaves seen through ops.
    int make_blas(const Ops& ops, const std::vector<int>& leaves, int bvh_node, int& rc)
    {
        const double pad_abs = pad_through(ops);
        int root;
        if (accel == RT_ACCEL_MEDIAN && bvh_node >= 0) {
            root = lower_ref_bvh(bvh_node, pad_abs, /*in_instance=*/true, rc);
            if (rc) return 0;
        } else {
            std::vector<Item> items;
            for (int hid : leaves) items.push_back(simple_item(hid, pad_abs));
            root = build_bvh(items, pad_abs, /*in_blas=*/true);
        }
        blas_depth = std::max(blas_depth, depth_of(root));
        return root;
    }

    // The leaves under a BVH node (through nested BvhNodes): simple ones and the rest.
    void collect_split(int id, std::vector<int>& simple, std::vector<int>& complex)
    {
        const HNode& h = w.nodes[id];
        if (h.kind == HKind::BvhNode) {
            collect_split(h.left, simple, complex);
            if (h.right != h.left) collect_split(h.right, simple, complex);  // span-1 duplicate
            return;
        }
        (is_simple(h.kind) ? simple : complex).push_back(id);
    }

    // Lowers the object `id` seen through the ops `prefix` into instance items.
    int lower_instance(int id, const Ops& prefix, std::vector<Item>& items)
    {
        Ops ops = prefix;
        int rc = RT_OK;
        const int child = chain(id, ops, rc);
        if (rc) return rc;
        const HNode& c = w.nodes[child];
        if (is_simple(c.kind)) {
            items.push_back(item_box(make_instance(ops, RT_CHILD_PRIM, lower_simple(child, pad_through(ops))),
                                     box_through(ops, bound_of(child)), /*costly=*/false));
            return RT_OK;
        }
        if (c.kind == HKind::ConstantMedium) return lower_medium(child, ops, items);
        if (c.kind != HKind::BvhNode) {
            err = "unsupported hittable under an instance";
            return RT_ERR_UNSUPPORTED;
        }
        std::vector<int> simple, complex;
        collect_split(child, simple, complex);
        if (!simple.empty()) {
            AABB b = bound_of(simple[0]);
            for (int hid : simple) b = hull(b, bound_of(hid));
            const int root = make_blas(ops, simple, complex.empty() ? child : -1, rc);
            if (rc) return rc;
            items.push_back(item_box(make_instance(ops, RT_CHILD_BVH, root), box_through(ops, b), /*costly=*/true));
        }
        for (int k : complex) {
            const HKind kk = w.nodes[k].kind;
            if (kk == HKind::Translate || kk == HKind::RotateY) rc = lower_instance(k, ops, items);
            else if (kk == HKind::ConstantMedium) rc = lower_medium(k, ops, items);
            else { err = "unsupported hittable under an instance"; rc = RT_ERR_UNSUPPORTED; }
            if (rc) return rc;
        }
        return RT_OK;
    }

    // ConstantMedium (hittable.rs:417-473) seen through ops: a medium primitive (boundary: a
    // primitive, or an instance over a primitive or a BLAS), itself the child of an instance
    // when ops is not empty.
    int lower_medium(int id, const Ops& ops, std::vector<Item>& items)
    {
        const HNode& h = w.nodes[id];
        int bprim;
        int rc = lower_boundary(h.ptr, bprim);
        if (rc) return rc;
        rt_prim p = blank(RT_PRIM_MEDIUM, h.mat - 1);
        p.a = bprim;
        p.b = h.medium_id;
        p.p[0] = h.neg_inv_density;
        const int mprim = add_prim(p);
        if (ops.n == 0) items.push_back(item_of(mprim, id, /*costly=*/true));
        else items.push_back(item_box(make_instance(ops, RT_CHILD_PRIM, mprim), box_through(ops, bound_of(id)), /*costly=*/false));
        return RT_OK;
    }

    // One primitive standing for a medium's boundary: a simple primitive, or an instance (a
    // Translate/RotateY chain, or none for a bare BvhNode) over a primitive or a BLAS. A
    // boundary holding instances or media below its chain is not lowered.
    int lower_boundary(int id, int& prim_out)
    {
        Ops ops;   // the boundary's own chain: the medium's space is padded as the world's
        if (is_simple(w.nodes[id].kind)) {
            prim_out = lower_simple(id, pad_through(ops));
            return RT_OK;
        }
        int rc = RT_OK;
        const int child = chain(id, ops, rc);
        if (rc) return rc;
        if (is_simple(w.nodes[child].kind)) {
            prim_out = make_instance(ops, RT_CHILD_PRIM, lower_simple(child, pad_through(ops)));
            return RT_OK;
        }
        if (w.nodes[child].kind == HKind::BvhNode) {
            std::vector<int> simple, complex;
            collect_split(child, simple, complex);
            if (complex.empty() && !simple.empty()) {
                const int root = make_blas(ops, simple, child, rc);
                if (rc) return rc;
                prim_out = make_instance(ops, RT_CHILD_BVH, root);
                return RT_OK;
            }
        }
        err = "a medium boundary holding instances or media is not lowered";
        return RT_ERR_UNSUPPORTED;
    }

    // MEDIAN mode: a reference BvhNode subtree lowered node for node (both child boxes from
    // bounding_box, hittable.rs:118-130); a non-BVH child becomes a one-primitive leaf.
    // A span-1 node (left == right, :100-102) tests the same leaf twice, as the reference does.
    int lower_ref_bvh(int id, double pad_abs, bool in_instance, int& rc)
    {
        const HNode& h = w.nodes[id];
        if (h.kind != HKind::BvhNode) {
            int prim = -1;
            if (is_simple(h.kind)) {
                prim = lower_simple(id, pad_abs);
            } else if (in_instance) {
                err = "instance over a BVH that contains an instance or a medium";
                rc = RT_ERR_UNSUPPORTED;
                return 0;
            } else {
                std::vector<Item> one;
                rc = lower_top(id, one);
                if (rc) return 0;
                prim = one[0].id;
            }
            const int first = (int)f.prim_refs.size();
            f.prim_refs.push_back(prim);
            return RT_LEAF_CODE(first, 1);
        }
        const int node = (int)f.nodes.size();
        f.nodes.emplace_back();
        const int lc = lower_ref_bvh(h.left, pad_abs, in_instance, rc);
        if (rc) return 0;
        const int rc_ref = h.right == h.left ? lc : lower_ref_bvh(h.right, pad_abs, in_instance, rc);
        if (rc) return 0;
        const Item li = item_box(lc, bound_of(h.left), false, true), ri = item_box(rc_ref, bound_of(h.right), false, true);
        rt_bvh_node& nd = f.nodes[node];
        std::memset(&nd, 0, sizeof nd);
        rtb::to_f32_box(li.lo, li.hi, pad_abs, nd.lo0, nd.hi0);
        rtb::to_f32_box(ri.lo, ri.hi, pad_abs, nd.lo1, nd.hi1);
        nd.child[0] = lc;
        nd.child[1] = rc_ref;
        return node;
    }

    int lower_top(int id, std::vector<Item>& items)
    {
        const HNode& h = w.nodes[id];
        switch (h.kind) {
        case HKind::BvhNode: {
            if (accel == RT_ACCEL_MEDIAN) {
                int rc = RT_OK;
                const int root = lower_ref_bvh(id, pad_through(Ops()), false, rc);
                if (rc) return rc;
                items.push_back(item_box(root, bound_of(id), false, /*subtree=*/true));
                return RT_OK;
            }
            int rc = lower_top(h.left, items);
            if (rc) return rc;
            if (h.right != h.left) return lower_top(h.right, items);
            return RT_OK;
        }
        case HKind::Translate: case HKind::RotateY: return lower_instance(id, Ops(), items);
        case HKind::ConstantMedium: return lower_medium(id, Ops(), items);
        default:
            items.push_back(simple_item(id, pad_through(Ops())));
            return RT_OK;
        }
    }
};

// The shading tables: materials, Perlin tables, image bytes and textures, as the world holds them.
void copy_shading_tables(const World& w, FlatScene& f)
{
    for (const Material& m : w.materials) {
        rt_material rm;
        std::memset(&rm, 0, sizeof rm);
        rm.kind = m.kind;
        rm.tex = m.tex;
        rm.albedo[0] = m.albedo.x; rm.albedo[1] = m.albedo.y; rm.albedo[2] = m.albedo.z;
        rm.fuzz = m.fuzz;
        rm.ir = m.ir;
        f.materials.push_back(rm);
    }
    for (const PerlinTables& p : w.perlins) {
        for (int i = 0; i < 256; ++i)
            for (int a = 0; a < 3; ++a) f.perlin_ranvec.push_back(p.ranvec[i][a]);
        for (int a = 0; a < 3; ++a)
            for (int i = 0; i < 256; ++i) f.perlin_perm.push_back(p.perm[a][i]);
    }
    std::vector<int64_t> img_off;
    for (const Image& im : w.images) {
        img_off.push_back((int64_t)f.image.size());
        f.image.insert(f.image.end(), im.rgb.begin(), im.rgb.end());
    }
    for (const Texture& t : w.textures) {
        rt_texture rt;
        std::memset(&rt, 0, sizeof rt);
        rt.kind = t.kind;
        rt.perlin = t.perlin;
        rt.c0[0] = t.c0.x; rt.c0[1] = t.c0.y; rt.c0[2] = t.c0.z;
        rt.c1[0] = t.c1.x; rt.c1[1] = t.c1.y; rt.c1[2] = t.c1.z;
        rt.scale = t.scale;
        if (t.kind == RT_TEX_IMAGE) {
            const Image& im = w.images[t.image];
            rt.img_w = im.rgb.empty() ? 0 : im.w;
            rt.img_h = im.rgb.empty() ? 0 : im.h;
            rt.img_offset = img_off[t.image];
            rt.img_bps = 3 * (int64_t)im.w;
        }
        f.textures.push_back(rt);
    }
}

// The sizes and pointers of f's tables (f where it will stay: the pointers are into its vectors).
void fill_soa(FlatScene& f)
{
    rt_scene_soa& s = f.soa;
    s.n_prims = (int32_t)f.prims.size();
    s.n_prim_refs = (int32_t)f.prim_refs.size();
    s.n_nodes = (int32_t)f.nodes.size();
    s.n_instances = (int32_t)f.instances.size();
    s.n_materials = (int32_t)f.materials.size();
    s.n_textures = (int32_t)f.textures.size();
    s.n_perlin = (int32_t)(f.perlin_perm.size() / (3 * 256));
    s.n_media = f.media;
    s.tlas_root = f.tlas_root;
    s.image_bytes = (int64_t)f.image.size();
    s.prims = f.prims.data();
    s.prim_refs = f.prim_refs.data();
    s.nodes = f.nodes.data();
    s.instances = f.instances.data();
    s.materials = f.materials.data();
    s.textures = f.textures.data();
    s.perlin_ranvec = f.perlin_ranvec.data();
    s.perlin_perm = f.perlin_perm.data();
    s.image_data = f.image.data();
}

}  // namespace

int flatten(World& w, int accel, std::string& err)
{
    if (accel != RT_ACCEL_SAH && accel != RT_ACCEL_LINEAR && accel != RT_ACCEL_MEDIAN) {
        err = "unknown accel mode";
        return RT_ERR_INVALID;
    }
    // the options (rt_world_set_build_option): the SAH builder's parameters, and the ray times the
    // boxes are built for (RT_BUILD_TIME0 / _TIME1; launch_plan.cpp refuses a camera whose shutter
    // leaves them when the scene holds a moving sphere)
    const BuildOptions& bo = w.build;
    if (!std::isfinite(bo.time0) || !std::isfinite(bo.time1)) {
        err = "build time range not finite";
        return RT_ERR_INVALID;
    }
    FlatScene f;
    Lowering low{w, f, err, accel,
                 rtb::sah_params(bo.c_isect, bo.max_leaf, bo.force_leaf, bo.root_leaf, bo.split_box_pairs, bo.split_blas_pairs),
                 std::min(bo.time0, bo.time1), std::max(bo.time0, bo.time1)};
    low.measure_extent();
    if (int rc = low.check_ref_bvhs()) return rc;
    // lower the top-level list (instances build their BLAS on the way) and build the TLAS over it
    std::vector<Item> top;
    for (int id : w.hittables) {
        if (!w.valid_hittable(id)) {
            err = "invalid hittable id in world list";
            return RT_ERR_INVALID;
        }
        if (int rc = low.lower_top(id, top)) return rc;
    }
    f.tlas_root = low.build_bvh(top, low.pad_through({}), /*in_blas=*/false);
    // the kernel's traversal stack: a TLAS walk, and a nested BLAS walk above it (<= 32 each)
    const int tlas_depth = low.depth_of(f.tlas_root);
    if (tlas_depth > 32 || low.blas_depth > 32) {
        err = "BVH too deep for the kernel's traversal stack";
        return RT_ERR_UNSUPPORTED;
    }
    const rtb::TlasFirst order = rtb::renumber_tlas_first(f.tlas_root, f.nodes, f.instances);
    f.tlas_root = order.root;
    f.media = w.n_media;
    copy_shading_tables(w, f);

    w.flat = std::move(f);
    rt_scene_soa& s = w.flat.soa;
    std::memset(&s, 0, sizeof s);
    fill_soa(w.flat);
    s.accel = accel;
    s.pad_extent = low.world_extent;
    s.time_lo = low.time_lo;
    s.time_hi = low.time_hi;
    s.tlas_depth = tlas_depth;
    s.n_tlas_nodes = order.n_tlas_nodes;
    s.blas_depth = low.blas_depth;
    return RT_OK;
}

}  // namespace rtw

