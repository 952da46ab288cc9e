// trace_walk.hpp — the megakernel's walk (third layer of trace_device.hpp): BVH nodes as read from
// LDS or L1/L2 and the block's LDS layout, traverse, Translate / RotateY instances, constant media,
// the hit record of the closest hit (finish_hit) and trace_world, one cast of a world-space ray.
#pragma once
#include "root_bracket.hpp"
#include "trace_prims.hpp"

namespace rtk {

// ---------------------------------------------------------------------------
// BVH traversal
// ---------------------------------------------------------------------------
constexpr int RT_DONE = (int)0x80000000;

// A node as four 16-B loads (ds_read_b128 from LDS, global_load_dwordx4 from L1/L2).
struct Node {
    float lo0[3], hi0[3], lo1[3], hi1[3];
    int child[2];
};
__device__ __forceinline__ Node load_node(const rt_bvh_node* base, int i)
{
    const uint4* q = reinterpret_cast<const uint4*>(base + i);
    const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
    Node n;
    n.lo0[0] = __uint_as_float(a.x); n.lo0[1] = __uint_as_float(a.y); n.lo0[2] = __uint_as_float(a.z);
    n.hi0[0] = __uint_as_float(a.w); n.hi0[1] = __uint_as_float(b.x); n.hi0[2] = __uint_as_float(b.y);
    n.lo1[0] = __uint_as_float(b.z); n.lo1[1] = __uint_as_float(b.w); n.lo1[2] = __uint_as_float(c.x);
    n.hi1[0] = __uint_as_float(c.y); n.hi1[1] = __uint_as_float(c.z); n.hi1[2] = __uint_as_float(c.w);
    n.child[0] = (int)d.x;
    n.child[1] = (int)d.y;
    return n;
}

// A node from LDS by byte address (four ds_read_b128 through an address-space-3 pointer: a
// generic pointer that may be LDS or global would be read with flat loads)
__device__ __forceinline__ Node load_node_lds(uint32_t addr);

// The TLAS node as staged in LDS by the variants whose whole TLAS is there and whose slab
// tests are f32 (OctNodes): per axis both children's lower planes, upper planes and the lower
// ones again, so a ray reads its near and far planes with one 16-B (2 x 8-B) read at an
// offset its direction sign selects (RayT::onx..onz); children as byte offsets of LdsNode
// (leaf codes unchanged). 80 B instead of rt_bvh_node's 64.
struct LdsNode {
    float ax[3][6];   // [axis][lo0 lo1 hi0 hi1 lo0 lo1]
    int32_t child[2];
};
static_assert(sizeof(LdsNode) == kLdsNodeBytes && sizeof(rt_bvh_node) == kBvhNodeBytes, "staged node records");
static_assert(sizeof(rt_material) == kMaterialBytes && sizeof(rt_texture) == kTextureBytes, "staged shading tables");
template <class C>
constexpr bool OctNodes() { return C::SHAPE.node_bytes == (int)sizeof(LdsNode); }
// LDS byte address of a __shared__ object (the low 32 bits of its flat address), and an LDS
// pointer from one: OctNodes node references are such addresses, so a node read needs no add
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)p; }
template <class T>
__device__ __forceinline__ const __attribute__((address_space(3))) T* lds_ptr(uint32_t a)
{
    return (const __attribute__((address_space(3))) T*)(uintptr_t)a;
}
template <class C>
constexpr int lds_node_bytes() { return C::SHAPE.node_bytes; }
__device__ __forceinline__ Node load_node_lds(uint32_t addr)
{
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
    const auto q = lds_ptr<u4v>(addr);
    const u4v a = q[0], b = q[1], c = q[2], d = q[3];
    Node n;
    n.lo0[0] = __uint_as_float(a.x); n.lo0[1] = __uint_as_float(a.y); n.lo0[2] = __uint_as_float(a.z);
    n.hi0[0] = __uint_as_float(a.w); n.hi0[1] = __uint_as_float(b.x); n.hi0[2] = __uint_as_float(b.y);
    n.lo1[0] = __uint_as_float(b.z); n.lo1[1] = __uint_as_float(b.w); n.lo1[2] = __uint_as_float(c.x);
    n.hi1[0] = __uint_as_float(c.y); n.hi1[1] = __uint_as_float(c.z); n.hi1[2] = __uint_as_float(c.w);
    n.child[0] = (int)d.x;
    n.child[1] = (int)d.y;
    return n;
}

// The material / texture table a shading step reads: staged in LDS by the block prologue
// (north_star: "stages the top BVH levels and material table in LDS") when the variant
// has rects or media and the tables are small (Cornell 4-6 materials, final scene 10), else
// global memory (the random scene's 485 materials would cost the spheres variant blocks per
// CU). The flag is per launch, so the choice is wave-uniform.
template <class C>
constexpr bool StageShade() { return C::SHAPE.stage_shade; }
// the variants that stage BLAS nodes (SceneDev.n_lds_blas; the host sets it only for them)
template <class C>
constexpr bool StageBlas() { return C::SHAPE.stage_blas; }
// The block's dynamic LDS (launch_shapes.hpp, lds_layout) of this configuration
template <class C>
__device__ __forceinline__ LdsLayout lds_layout_of(const SceneDev& S)
{
    return lds_layout(S.n_lds_nodes, lds_node_bytes<C>(), StageBlas<C>() ? S.n_lds_blas : 0, C::LDS ? S.stack_entries : 0,
                      C::SHAPE.entry_bytes, StageShade<C>() ? S.n_lds_materials : 0,
                      StageShade<C>() ? S.n_lds_textures : 0, BlockThreads<C>());
}

// Closest hit in a BVH (nodes + leaf ranges of slots j, whose records are leaf_prims[j]).
// `leaf(slot, t_max, best)` tests one primitive; on a closer hit it fills best (t and sub
// ids) and returns true; best.prim is then the slot.
// CfgDefer's top-level walk (DEFER): best is an rtrb::Best, the slot and an f32 bracket of its
// exact t, which `leaf(slot, best)` updates itself; the walk carries no f64 t_max, and prunes by the
// bracket's upper end (conservative, and strictly above the exact t: a tie is never pruned).
template <class C, bool NL = false, class LeafFn, class R = typename C::Real, class Best = HitRefT<R>>
__device__ __forceinline__ bool traverse(const SceneDev& S, int root, const RayT<R>& r, R t_min, R t_max,
                                         Best& best, StackT<C>& stack, int sp0, Count& cnt, LeafFn&& leaf)
{
    constexpr bool DEFER = C::DEFER && NL && std::is_same<Best, rtrb::Best>::value;
    static_assert(!DEFER || C::S32, "deferred roots: the f32-slab kernels");
    // NL: this is the TLAS, whose first S.n_lds_nodes nodes (BFS order) were copied into
    // LDS at block start; deeper nodes are read from L1/L2
    const rt_bvh_node* lds_nodes =
        reinterpret_cast<const rt_bvh_node*>(rt_lds);   // at LDS address 0: node offsets are addresses
    bool any = false;
    // the walk's bottom entry is RT_DONE (the host reserves it: SceneDev.stack_entries,
    // blas_base), so a pop needs no empty-stack test: popping it ends the walk
    constexpr int DONE = Stack16Cfg<C>() ? -32768 : RT_DONE;   // the walk's bottom entry
    // the stack pointer as an address, pre-scaled by the entry stride: a push or pop is one
    // add (not an add plus a shift-add of the index)
    constexpr int SSTR = C::LDS ? BlockThreads<C>() : 1;
    auto* sptr = &stack[sp0];
    using SE = typename std::remove_reference<decltype(*sptr)>::type;
    *sptr = (SE)DONE;
    sptr += SSTR;
    auto push = [&](int v) { *sptr = (SE)v; sptr += SSTR; };
    auto pop = [&]() -> int { sptr -= SSTR; return (int)*sptr; };
    int cur = root;
    float tmin_f = 0.0f, tmax_f = 0.0f;
    if constexpr (C::S32) {
        tmin_f = f32_down(t_min);
        tmax_f = f32_up(t_max);
    }
    if constexpr (DEFER) tmax_f = best.hi;   // (the pre-leaf's hit, or +inf)
    // TLAS entirely in LDS, f32 slabs (OctNodes): the node is the 80-B LdsNode layout and
    // node references are byte offsets; per axis one 16-B read at the offset the ray's
    // direction sign selects gives both children's near planes, then their far planes, so
    // the slab test needs no min/max pair per axis: t_near = max(near planes), t_far =
    // min(far planes). One address add per axis, the child pair at a fixed offset.
    constexpr bool OCT = NL && OctNodes<C>();
    float ninf = -__builtin_inff();
    if constexpr (OCT) asm("s_mov_b32 %0, 0xff800000" : "=s"(ninf));
    const char* const lb = reinterpret_cast<const char*>(lds_nodes);
    uint32_t blas_lds_base = 0;   // LDS byte address of the staged BLAS nodes (nested walks)
    if constexpr (!NL && StageBlas<C>()) blas_lds_base = lds_addr(lb) + (uint32_t)lds_layout_of<C>(S).blas;
    (void)blas_lds_base;
    if constexpr (OCT) cur = cur >= 0 ? (int)(lds_addr(lb) + (uint32_t)cur * (uint32_t)sizeof(LdsNode)) : cur;
    // one node visit: test both children, continue with the nearer, push the farther
    auto visit = [&](int node) -> int {
        if (C::COUNT) cnt.nodes++;
        if constexpr (OCT) {
            const uint32_t nb = (uint32_t)node;   // LDS address of the node
            typedef float f2v __attribute__((ext_vector_type(2)));
            typedef int i2v __attribute__((ext_vector_type(2)));
            auto pairs = [&](uint32_t off, f2v& n, f2v& f) {
                const auto q = lds_ptr<f2v>(nb + off);   // one ds_read2_b64
                n = q[0];
                f = q[1];
            };
            f2v npx, fpx, npy, fpy, npz, fpz;
            pairs(r.onx, npx, fpx);
            pairs(r.ony, npy, fpy);
            pairs(r.onz, npz, fpz);
            const i2v ch = *lds_ptr<i2v>(nb + (uint32_t)offsetof(LdsNode, child));
            float tn[2], tf[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const float nx = __builtin_fmaf(c ? npx.y : npx.x, r.sx.x, r.sx.y);
                const float ny = __builtin_fmaf(c ? npy.y : npy.x, r.sy.x, r.sy.y);
                const float nz = __builtin_fmaf(c ? npz.y : npz.x, r.sz.x, r.sz.y);
                const float fx = __builtin_fmaf(c ? fpx.y : fpx.x, r.sx.x, r.sx.y);
                const float fy = __builtin_fmaf(c ? fpy.y : fpy.x, r.sy.x, r.sy.y);
                const float fz = __builtin_fmaf(c ? fpz.y : fpz.x, r.sz.x, r.sz.y);
                tn[c] = fmaxf(fmaxf(nx, ny), fmaxf(nz, tmin_f));
                // min(fz, t_max) as v_med3(fz, t_max, -inf): fminf would re-quiet the loop-carried
                // t_max (a v_max_f32 t, t) at every visit; the plane products are never NaN.
                // (-inf from an SGPR: with the constant the compiler folds med3 back to fminf.)
                tf[c] = fminf(fminf(fx, fy), __builtin_amdgcn_fmed3f(fz, tmax_f, ninf));
            }
            const bool h0 = tn[0] <= tf[0], h1 = tn[1] <= tf[1], near0 = tn[0] <= tn[1];
            if (h0 && h1) {
                push(near0 ? ch.y : ch.x);
                return near0 ? ch.x : ch.y;
            }
            if (h0) return ch.x;
            if (h1) return ch.y;
            return pop();
        }
        Node nd;
        if constexpr (!NL && StageBlas<C>()) {
            // a nested (BLAS) walk: its staged top levels from LDS (ds_read_b128 through an LDS
            // pointer), the rest from L1/L2
            const uint32_t j = (uint32_t)(node - S.n_tlas_nodes);
            if (j < (uint32_t)S.n_lds_blas) nd = load_node_lds(blas_lds_base + j * (uint32_t)sizeof(rt_bvh_node));
            else nd = load_node(S.nodes, node);
        } else {
            nd = (NL && (C::NALL || node < S.n_lds_nodes)) ? load_node(lds_nodes, node) : load_node(S.nodes, node);
        }
        bool h0, h1, near0;
        if constexpr (C::S32) {
            float tn0, tn1;
            h0 = slab32(nd.lo0, nd.hi0, r, tmin_f, tmax_f, tn0);
            h1 = slab32(nd.lo1, nd.hi1, r, tmin_f, tmax_f, tn1);
            near0 = tn0 <= tn1;
        } else {
            R tn0, tn1;
            h0 = slab(nd.lo0, nd.hi0, r, t_min, t_max, tn0);
            h1 = slab(nd.lo1, nd.hi1, r, t_min, t_max, tn1);
            near0 = tn0 <= tn1;
        }
        if (h0 && h1) {
            push(near0 ? nd.child[1] : nd.child[0]);
            return near0 ? nd.child[0] : nd.child[1];
        }
        if (h0) return nd.child[0];
        if (h1) return nd.child[1];
        return pop();
    };
    auto do_leaf = [&](int code) {
        code = ~code;
        const int first = code >> 5, count = code & 31;
        for (int i = 0; i < count; ++i) {
            if (C::COUNT && first_active_lane()) cnt.wave_leaves++;
            const int slot = first + i;
            if constexpr (DEFER) {
                if (leaf(slot, best)) tmax_f = best.hi;
            } else if (leaf(slot, t_max, best)) {
                best.prim = slot;
                t_max = best.t;
                any = true;
                if constexpr (C::S32) tmax_f = f32_up(t_max);
            }
        }
    };
    uint64_t t0 = 0;
    while (cur != DONE) {
        if (C::COUNT && NL) t0 = __builtin_amdgcn_s_memtime();
        while (cur >= 0) {
            if (C::COUNT && first_active_lane()) cnt.wave_nodes++;
            cur = visit(cur);
        }
        if (NL) RT_STAMP(cnt.t_nodes, t0);   // the TLAS walk only: a nested walk is part of its leaf
        if (cur == DONE) break;
        do_leaf(cur);
        cur = pop();
        if (NL) RT_STAMP(cnt.t_leaves, t0);
    }
    if constexpr (DEFER) return best.prim >= 0;
    return any;
}

// ---------------------------------------------------------------------------
// Translate / RotateY instances (hittable.rs:232-244, 386-415), outermost op first
// ---------------------------------------------------------------------------
template <class R>
__device__ __forceinline__ void instance_ray(const rt_instance& in, RayT<R>& r)
{
    const int n = in.n_ops;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < n) {
            if (in.op_kind[i] == RT_OP_TRANSLATE) {  // moved_ray = (o - offset, d, time)
                r.ox = r.ox - (R)in.op[i][0];
                r.oy = r.oy - (R)in.op[i][1];
                r.oz = r.oz - (R)in.op[i][2];
            } else {                                  // rotated_ray
                const R s = (R)in.op[i][0], c = (R)in.op[i][1];
                const R ox = c * r.ox - s * r.oz, oz = s * r.ox + c * r.oz;
                const R dx = c * r.dx - s * r.dz, dz = s * r.dx + c * r.dz;
                r.ox = ox; r.oz = oz; r.dx = dx; r.dz = dz;
            }
        }
    }
}

template <class C, class R = typename C::Real>
__device__ bool medium_t(const SceneDev& S, const rt_prim& m, const RayT<R>& r, R t_min, R t_max, R& t,
                         StackT<C>& stack, int sp0, const Keyed& key, Count& cnt);
template <class R>
__device__ __forceinline__ void medium_finish(const rt_prim& m, const RayT<R>& r, R t, HitT<R>& h);

// t-only: the closest hit of the instance's child; sub = BLAS prim (or the child prim),
// side = winning box side.
template <class C, class R = typename C::Real>
__device__ bool instance_t(const SceneDev& S, const rt_instance& in, const RayT<R>& ray, R t_min, R t_max,
                           HitRefT<R>& ref, StackT<C>& stack, int sp0, const Keyed& key, Count& cnt)
{
    RayT<R> r = ray;
    instance_ray(in, r);
    if (in.child_kind == RT_CHILD_PRIM) {
        if constexpr ((C::F & FEAT_INST_MEDIUM) != 0) {
            const rt_prim& cp = S.prims[in.child];
            if (cp.kind == RT_PRIM_MEDIUM) {   // the medium in object space (its boundary walks at sp0)
                finish_ray<C>(r, S.has_spheres != 0);
                if (!medium_t<InstMedC<C>>(S, cp, r, t_min, t_max, ref.t, stack, sp0, key, cnt)) return false;
                ref.sub = in.child;
                ref.side = 0;
                return true;
            }
        }
        // one primitive: no node-slab terms
        finish_ray<C, false>(r, S.has_spheres != 0);
        int side = 0;
        if (!simple_t<InstC<C>>(S.prims[in.child], r, t_min, t_max, ref.t, side, cnt, (C::F & FEAT_SHUTTER) != 0)) return false;
        ref.sub = in.child;
        ref.side = side;
        return true;
    }
    // an instance over a BVH: a nested walk (its state on top of the TLAS walk's is what
    // set the Cornell variants' register count, 157 vs 125 VGPRs: 3 vs 4 waves per SIMD)
    if constexpr ((C::F & FEAT_INST_BLAS) == 0) return false;
    finish_ray<C>(r, S.has_spheres != 0);
    HitRefT<R> inner;
    const rt_prim* const blas_prims = S.leaf_prims + in.pad;   // the BLAS's leaf codes count from its first slot
    if (!traverse<C>(S, in.child, r, t_min, t_max, inner, stack, sp0, cnt,
                     [&](int slot, R tmax, HitRefT<R>& b) {
                         return simple_t<InstC<C>>(blas_prims[slot], r, t_min, tmax, b.t, b.side, cnt, (C::F & FEAT_SHUTTER) != 0);
                     }))
        return false;
    ref.t = inner.t;
    ref.sub = in.pad + inner.prim;   // absolute leaf slot (instance_finish)
    ref.side = inner.side;
    return true;
}

// The ray direction after ops 0..i (only RotateY changes it; y never changes): recomputed
// per op on the way back instead of kept in arrays through the child's finisher, which
// held 8 f64 registers live and pushed the instance variants into scratch spills.
template <class R>
__device__ __forceinline__ void dir_after(const rt_instance& in, const RayT<R>& ray, int i, R& dx, R& dz)
{
    dx = ray.dx;
    dz = ray.dz;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j <= i && j < in.n_ops && in.op_kind[j] != RT_OP_TRANSLATE) {
            const R s = (R)in.op[j][0], c = (R)in.op[j][1];
            const R x = c * dx - s * dz, z = s * dx + c * dz;
            dx = x;
            dz = z;
        }
    }
}

template <class C, class R = typename C::Real>
__device__ void instance_finish(const SceneDev& S, const rt_instance& in, const RayT<R>& ray, const HitRefT<R>& ref,
                                HitT<R>& h)
{
    RayT<R> r = ray;
    instance_ray(in, r);
    // ref.sub: the child prim (RT_CHILD_PRIM) or the BLAS leaf slot
    bool done = false;
    if constexpr ((C::F & FEAT_INST_MEDIUM) != 0) {
        if (in.child_kind == RT_CHILD_PRIM && S.prims[ref.sub].kind == RT_PRIM_MEDIUM) {
            medium_finish(S.prims[ref.sub], r, ref.t, h);   // hittable.rs:452-463 in object space
            done = true;
        }
    }
    if (!done)
        simple_finish<InstC<C>>((C::F & FEAT_INST_BLAS) == 0 || in.child_kind == RT_CHILD_PRIM ? S.prims[ref.sub]
                                                                                               : S.leaf_prims[ref.sub],
                                r, ref.t, ref.side, h, (C::F & FEAT_SHUTTER) != 0);
    const int n = in.n_ops;
#pragma unroll
    for (int i = 3; i >= 0; --i) {
        if (i < n) {
            R dx, dz;
            dir_after(in, ray, i, dx, dz);
            if (in.op_kind[i] == RT_OP_TRANSLATE) {  // rec.point += offset; set_face_normal(moved_ray, normal)
                h.px = h.px + (R)in.op[i][0];
                h.py = h.py + (R)in.op[i][1];
                h.pz = h.pz + (R)in.op[i][2];
                set_face_normal(h, dx, ray.dy, dz, h.nx, h.ny, h.nz);
            } else {                                  // rotate back; set_face_normal(rotated_ray, normal)
                const R s = (R)in.op[i][0], c = (R)in.op[i][1];
                const R px = c * h.px + s * h.pz, pz = -s * h.px + c * h.pz;
                const R nx = c * h.nx + s * h.nz, nz = -s * h.nx + c * h.nz;
                h.px = px; h.pz = pz;
                set_face_normal(h, dx, ray.dy, dz, nx, h.ny, nz);
            }
        }
    }
}

// t of a medium boundary (a simple prim or an instance).
template <class C, class R = typename C::Real>
__device__ __forceinline__ bool boundary_t(const SceneDev& S, int prim, const RayT<R>& r, R t_min, R t_max, R& t,
                                           StackT<C>& stack, int sp0, const Keyed& key, Count& cnt)
{
    const rt_prim& p = S.prims[prim];
    if constexpr ((BoundC<C>::F & FEAT_INST) != 0) {
        if (p.kind == RT_PRIM_INSTANCE) {
            HitRefT<R> ref;
            if (!instance_t<BoundC<C>>(S, S.instances[p.a], r, t_min, t_max, ref, stack, sp0, key, cnt)) return false;
            t = ref.t;
            return true;
        }
    }
    int side = 0;
    return simple_t<BoundC<C>>(p, r, t_min, t_max, t, side, cnt, (C::F & FEAT_SHUTTER) != 0);
}

// ConstantMedium (hittable.rs:417-473), keyed draw instead of the in-hit thread_rng().
template <class C, class R>
__device__ bool medium_t(const SceneDev& S, const rt_prim& m, const RayT<R>& r, R t_min, R t_max, R& t,
                         StackT<C>& stack, int sp0, const Keyed& key, Count& cnt)
{
    R t1, t2;
    if constexpr ((BoundC<C>::F & (FEAT_INST | FEAT_RECT)) == 0) {
        // every medium boundary of this variant is a sphere: both queries from one quadratic
        const rt_prim& p = S.prims[m.a];
        if (C::COUNT) cnt.prims += 2;
        double cx, cy, cz;
        sphere_center(p, r, (C::F & FEAT_SHUTTER) != 0, cx, cy, cz, (BoundC<C>::F & FEAT_STATIC) != 0);
        if (!sphere_t2(cx, cy, cz, p.p[3], r, t1, t2)) return false;
    } else {
        if (!boundary_t<C>(S, m.a, r, (R)-RT_INF, (R)RT_INF, t1, stack, sp0, key, cnt)) return false;
        // the second boundary hit after t1 + 0.0001 (hittable.rs:433); in f32 the step must
        // also clear t1's own rounding (a fog sphere of r = 5000 has ulp(t1) = 4.9e-4 > 1e-4)
        R t1_next = t1 + (R)0.0001;
        if constexpr (C::F32) t1_next = t1 + fmaxf(0.0001f, __builtin_fabsf(t1) * 0x1.0p-19f);
        if (!boundary_t<C>(S, m.a, r, t1_next, (R)RT_INF, t2, stack, sp0, key, cnt)) return false;
    }
    if (t1 < t_min) t1 = t_min;
    if (t2 > t_max) t2 = t_max;
    if (t1 >= t2) return false;
    if (t1 < (R)0) t1 = (R)0;
    const R ray_length = r_sqrt(r.a);
    const R distance_inside = (t2 - t1) * ray_length;
    const uint64_t bits = rt_keyed_u64(key.seed, key.pixel, key.sample, key.bounce, RT_STREAM_MEDIUM + (uint32_t)m.b);
    R xi;
    if constexpr (C::F32) xi = (float)(bits >> 40) * 0x1.0p-24f;   // [0, 1) in 2^-24 steps
    else xi = rt_unit53(bits);
    const R hit_distance = (R)m.p[0] * r_log(xi);
    if (hit_distance > distance_inside) return false;
    t = t1 + hit_distance / ray_length;
    return true;
}

// hittable.rs:452-463
template <class R>
__device__ __forceinline__ void medium_finish(const rt_prim& m, const RayT<R>& r, R t, HitT<R>& h)
{
    h.t = t;
    h.px = r.ox + r.dx * t;
    h.py = r.oy + r.dy * t;
    h.pz = r.oz + r.dz * t;
    h.nx = (R)1; h.ny = (R)0; h.nz = (R)0;
    h.front = 1;
    h.mat = m.mat;
    h.uvkind = 0;
}

// The HitRecord of the closest hit (t, leaf slot, sub-primitive, box side) of a world-space ray:
// the arithmetic of the winning primitive's hit (hittable.rs:254-384, 417-473) and of the
// instance chain back to world space (hittable.rs:232-244, 386-415). Traversal keeps only the
// reference; the record is built once per cast (trace_world).
template <class C, class R = typename C::Real>
__device__ __forceinline__ void finish_hit(const SceneDev& S, const RayT<R>& r, const HitRefT<R>& best, HitT<R>& h)
{
    const rt_prim& p = S.leaf_prims[best.prim];
    bool done = false;
    if constexpr ((C::F & FEAT_INST) != 0) {
        if (p.kind == RT_PRIM_INSTANCE) {
            instance_finish<C>(S, S.instances[p.a], r, best, h);
            done = true;
        }
    }
    if constexpr ((C::F & FEAT_MEDIUM) != 0) {
        if (!done && p.kind == RT_PRIM_MEDIUM) {
            medium_finish(p, r, best.t, h);
            done = true;
        }
    }
    if (!done) simple_finish<C>(p, r, best.t, best.side, h, (C::F & FEAT_SHUTTER) != 0);
}

// The variants that test SceneDev.pre_leaf before the walk: the spheres ones (random scene:
// C2 19.17 -> 17.70 ms); the final scene gains nothing (its fog medium's test inlined twice
// spills) and the Cornell variant would drop to 3 waves per SIMD.
template <class C>
constexpr bool PreLeaf() { return C::F == FEAT_SET_SPHERES; }
// the variants whose instances can hold a BLAS (a nested walk) defer their first instance test
template <class C>
constexpr bool DeferInst() { return RT_DEFER_INST && (C::F & FEAT_INST_BLAS) != 0; }

// The variants that walk a one-leaf top level (the Cornell scenes: S.tlas_root is a leaf code) as
// a plain loop over its slots: no stack, no node loop, a loop count the same in every lane (scalar
// control instead of exec-masked loops). Measured: C3 800x800x200 45.71 -> 41.88 ms, Cornell smoke
// 57.80 -> 52.50, same images; making the kind and instance index wave-uniform on top (scalar
// dispatch) was slower (42.51 / 52.80; profiles/r04q_ab_*.log, r04r_ab_*.log). Not in the variants
// with nested BLAS walks (the final and all-features ones keep their register allocation); the
// spheres variants take the pre-leaf path.
template <class C>
constexpr bool UniformLeaf() { return (C::F & FEAT_INST_BLAS) == 0 && !PreLeaf<C>(); }

// CfgDefer (root_bracket.hpp): the exact root of leaf slot `slot`'s sphere over [t_min, +inf), in
// sphere_t's arithmetic, and the deferred test of one candidate against the best so far.
template <class C>
__device__ __forceinline__ bool sphere_exact_of(const SceneDev& S, const RayT<double>& r, int slot, double t_min, double& t)
{
    static_assert((C::F & FEAT_RECT) == 0 && !C::F32, "deferred roots: the f64 spheres variant");
    const rt_prim& p = S.leaf_prims[slot];
    double cx, cy, cz, half_b, disc;
    sphere_center(p, r, (C::F & FEAT_SHUTTER) != 0, cx, cy, cz, (C::F & FEAT_STATIC) != 0);
    sphere_quad(cx, cy, cz, p.p[3], r, half_b, disc);
    if (disc < 0.0) return false;
    return sphere_root(half_b, disc, r, t_min, t);
}
template <class C>
__device__ __forceinline__ bool sphere_defer_t(const SceneDev& S, const RayT<double>& r, float yaf, int slot, double t_min,
                                               rtrb::Best& best)
{
    static_assert((C::F & FEAT_RECT) == 0 && !C::F32, "deferred roots: the f64 spheres variant");
    const rt_prim& p = S.leaf_prims[slot];
    double cx, cy, cz, half_b, disc;
    sphere_center(p, r, (C::F & FEAT_SHUTTER) != 0, cx, cy, cz, (C::F & FEAT_STATIC) != 0);
    sphere_quad(cx, cy, cz, p.p[3], r, half_b, disc);
    if (disc < 0.0) return false;   // the sign of disc stays exact
    return rtrb::closer(
        best, slot, half_b, disc, yaf, rtrb::down(t_min), rtrb::up(t_min),
        [&](double& t) { return sphere_root(half_b, disc, r, t_min, t); },
        [&](int s, double& t) { return sphere_exact_of<C>(S, r, s, t_min, t); });
}

// trace_world of the CfgDefer kernels: the pre-leaf (the ground sphere, one converged test per
// cast) stays exact and seeds the bracket; the walk's leaf tests decide from brackets; the winner's
// exact root — today's bits: the root a sphere is accepted with does not depend on t_max — is
// computed once, by every hit lane together, before the hit record.
template <class C>
__device__ __forceinline__ bool trace_world_defer(const SceneDev& S, const RayT<double>& r, HitT<double>& h, StackT<C>& stack,
                                                  Count& cnt)
{
    static_assert(PreLeaf<C>() && C::S32 && !C::COUNT, "deferred roots: the f64 spheres variant's timed kernels");
    const double t_min = 0.001;
    rtrb::Best best = rtrb::none();
    const float yaf = rtrb::ya32(r.ya);   // the ray's part of every bracket
    int root = S.tlas_root;
    if (S.pre_leaf != 0) {   // (wave-uniform)
        root = S.pre_root;
        float tn;
        if (slab32(S.pre_lo, S.pre_hi, r, f32_down(t_min), f32_up(RT_INF), tn)) {
            const int code = ~S.pre_leaf;
            double t_max = RT_INF;
            for (int slot = code >> 5, end = (code >> 5) + (code & 31); slot < end; ++slot) {
                double t;
                if (sphere_exact_of<C>(S, r, slot, t_min, t) && !(t_max < t)) {
                    best.prim = slot;
                    t_max = t;
                }
            }
            if (best.prim >= 0) {
                best.lo = f32_down(t_max);
                best.hi = f32_up(t_max);
            }
        }
    }
    if (!traverse<C, true>(S, root, r, t_min, RT_INF, best, stack, 0, cnt,
                           [&](int slot, rtrb::Best& b) { return sphere_defer_t<C>(S, r, yaf, slot, t_min, b); }))
        return false;
    HitRefT<double> ref;
    ref.prim = best.prim;
    ref.sub = 0;
    ref.side = 0;
    (void)sphere_exact_of<C>(S, r, best.prim, t_min, ref.t);
    finish_hit<C>(S, r, ref, h);
    return true;
}

// hit_hittables(world, ray, 0.001, inf) (hittable.rs:43-55) over the TLAS, then the HitRecord of
// the closest primitive.
template <class C, class R = typename C::Real>
__device__ bool trace_world(const SceneDev& S, const RayT<R>& r, HitT<R>& h, StackT<C>& stack, const Keyed& key,
                            Count& cnt)
{
    if constexpr (C::DEFER) return trace_world_defer<C>(S, r, h, stack, cnt);
    const R t_min = (R)0.001;
    HitRefT<R> best;
    best.sub = 0;
    best.side = 0;
    // DeferInst: the first instance a lane's walk reaches is tested after the walk (pend), so
    // the lanes of a wave that have one walk its BLAS together, once, instead of each at its
    // own step of the top-level walk while the others wait; its t_max is then the walk's final
    // closest hit, which prunes it further. Closest hit does not depend on the order of the
    // tests (the instance's t is the ray's t), so the image does not change.
    int pend = -1;
    (void)pend;
    auto leaf = [&](int slot, R tmax, HitRefT<R>& b) {
        const rt_prim& p = S.leaf_prims[slot];
        if constexpr ((C::F & FEAT_INST) != 0)
            if (p.kind == RT_PRIM_INSTANCE) {
                if constexpr (DeferInst<C>()) {
                    if (pend < 0 && p.b != 0) {   // (b: its child is a BVH, upload)
                        pend = slot;
                        return false;
                    }
                }
                uint64_t ti = 0;
                if (C::COUNT) ti = __builtin_amdgcn_s_memtime();
                const bool hit = instance_t<C>(S, S.instances[p.a], r, t_min, tmax, b, stack, S.blas_base, key, cnt);
                RT_STAMP(cnt.t_inst, ti);
                return hit;
            }
        if constexpr ((C::F & FEAT_MEDIUM) != 0)
            if (p.kind == RT_PRIM_MEDIUM) {
                uint64_t tm = 0;
                if (C::COUNT) tm = __builtin_amdgcn_s_memtime();
                const bool hit = medium_t<C>(S, p, r, t_min, tmax, b.t, stack, S.blas_base, key, cnt);
                RT_STAMP(cnt.t_med, tm);
                return hit;
            }
        return simple_t<C>(p, r, t_min, tmax, b.t, b.side, cnt, (C::F & FEAT_SHUTTER) != 0);
    };
    uint64_t tp = 0;
    if (C::COUNT) tp = __builtin_amdgcn_s_memtime();
    bool hit;
    if constexpr (PreLeaf<C>()) {
        R t_max = (R)RT_INF;
        hit = false;
        int root = S.tlas_root;
        if (S.pre_leaf != 0) {   // wave-uniform: the huge root-child leaf first (SceneDev.pre_leaf)
            root = S.pre_root;
            bool in_box;
            if constexpr (C::S32) {
                float tn;
                in_box = slab32(S.pre_lo, S.pre_hi, r, f32_down(t_min), f32_up(t_max), tn);
            } else {
                R tn;
                in_box = slab(S.pre_lo, S.pre_hi, r, t_min, t_max, tn);
            }
            if (in_box) {
                const int code = ~S.pre_leaf;
                for (int slot = code >> 5, end = (code >> 5) + (code & 31); slot < end; ++slot) {
                    if (leaf(slot, t_max, best)) {
                        best.prim = slot;
                        t_max = best.t;
                        hit = true;
                    }
                }
            }
        }
        if (S.pre_leaf != 0) root = S.pre_root;
        RT_STAMP(cnt.t_pre, tp);
        hit |= traverse<C, true>(S, root, r, t_min, t_max, best, stack, 0, cnt, leaf);
    } else {
        RT_STAMP(cnt.t_pre, tp);
        if (UniformLeaf<C>() && S.tlas_root < 0 && S.tlas_root != RT_DONE) {   // (wave-uniform)
            const int code = ~S.tlas_root;
            R t_max = (R)RT_INF;
            hit = false;
            uint64_t tl = 0;
            if (C::COUNT) tl = __builtin_amdgcn_s_memtime();
            for (int slot = code >> 5, end = (code >> 5) + (code & 31); slot < end; ++slot) {
                if (C::COUNT && first_active_lane()) cnt.wave_leaves++;
                if (leaf(slot, t_max, best)) {   // traverse's do_leaf, in slot order
                    best.prim = slot;
                    t_max = best.t;
                    hit = true;
                }
            }
            RT_STAMP(cnt.t_leaves, tl);
        } else {
            hit = traverse<C, true>(S, S.tlas_root, r, t_min, (R)RT_INF, best, stack, 0, cnt, leaf);
        }
    }
    if (C::COUNT) tp = __builtin_amdgcn_s_memtime();   // the walk stamped its own phases
    if constexpr (DeferInst<C>()) {
        if (pend >= 0) {
            const rt_prim& p = S.leaf_prims[pend];
            HitRefT<R> b;
            b.sub = 0;
            b.side = 0;
            // the top-level walk is done: its stack is free, the BLAS walk starts at entry 0
            if (instance_t<C>(S, S.instances[p.a], r, t_min, hit ? best.t : (R)RT_INF, b, stack, 0, key, cnt)) {
                best = b;
                best.prim = pend;
                hit = true;
            }
            RT_STAMP(cnt.t_defer, tp);
        }
        if (C::COUNT) tp = __builtin_amdgcn_s_memtime();   // lanes without one
    }
    if (!hit) return false;
    finish_hit<C>(S, r, best, h);
    RT_STAMP(cnt.t_rec, tp);
    return true;
}

}  // namespace rtk
