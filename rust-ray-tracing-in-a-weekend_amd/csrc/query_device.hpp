// query_device.hpp — rt_trace_rays' kernel (include/rt/rt_abi.h): the closest hit, or whether there
// is any, of rays read from memory, over the megakernel's device functions (trace_shade.hpp and the
// layers below it: traverse, instance_t, medium_t, simple_t, finish_hit, tex_value, stage_lds). Like
// features_device.hpp it includes neither schedule, and only the query_v_*.hip translation units
// and query_kernel.hip include it; the trace and feature variants hold none of it.
//
// trace_features' construction with the ray read from an rt_ray record instead of made by
// camera_ray, and the interval taken from the ray instead of fixed at (0.001, inf): one lane per
// ray, ray blockIdx.x * BlockThreads + threadIdx.x. A few compares decide whether the ray is walked
// at all (rt_abi.h, "Invalid rays"): a bad input ends as a flag, never as a long walk. Records are
// 80 bytes and 16-byte aligned, read and written as five 16-byte vector loads and stores; the albedo
// and occlusion outputs are plain vector stores too. No atomics.
//
// Launch bounds, waves per SIMD and the LDS layout are the trace kernel's of the same
// configuration (Cfg::SHAPE, lds_layout). One number of the layout is the query's own: its stack
// holds the entries of a walk that nests every BLAS walk (SceneFacts.nested_stack_entries; the
// driver plans and launches with it), because this walk defers no instance and the scene's
// stack_entries may count on the trace kernels' deferral.
#pragma once
#include "trace_shade.hpp"
#include "trace_grid.hpp"
#include "trace_launch_common.hpp"
#include "query_kernel.hpp"

namespace rtk {

static_assert(sizeof(rt_ray) == 80 && sizeof(rt_hit) == 80, "five 16-byte words per record");

// hit_hittables(world, ray, t_min, t_max) (hittable.rs:43-55) over the TLAS from S.tlas_root, both
// interval ends the caller's and handed to every primitive test unchanged: trace_world's leaf
// tests (instance_t / medium_t / simple_t) and its one-leaf top-level loop (UniformLeaf), without
// its two scheduling devices — the pre-leaf hoist and the deferred instance reorder the tests of a
// bounce loop's casts, and a walk from the root is complete without them (closest hit does not
// depend on the order of the tests). Every instance is tested where the walk meets it, its BLAS
// walk at S.blas_base above the top-level walk's entries: the stack must hold both. Returns whether a test accepted; best is then the closest
// hit's reference for finish_hit.
//
// ANY stops at the first test that accepts. That is "CLOSEST would report a hit": until a first
// test accepts, both walks run the same tests with the same t_max, the caller's, so one accepts
// exactly when the other does, and after it CLOSEST can only replace its hit by a closer one.
// Across acceleration structures, which reach the primitives in other orders, a test may see a
// smaller t_max than the caller's only after another test has accepted; and a medium, the one
// primitive whose answer is drawn, draws one keyed number per ray and accepts with the same t
// under any larger t_max, so no order turns a ray with an accepted test into one without.
// The exit needs nothing of traverse: the accepting leaf hands back t = -inf, which becomes the
// walk's t_max, below every t_min; every later slab test fails, every later leaf returns at once
// (found), and the stack drains by pops alone. (With t_min = -inf a slab test can still pass; the
// leaves below it return at once, so the answer stands.)
template <class C, bool ANY, class R = typename C::Real>
__device__ __forceinline__ bool cast_interval(const SceneDev& S, const RayT<R>& r, R t_min, R t_max, HitRefT<R>& best,
                                              StackT<C>& stack, const Keyed& key, Count& cnt)
{
    best.sub = 0;
    best.side = 0;
    bool found = false, have = false;   // ANY: a test accepted; CLOSEST: best holds a hit
    (void)found;
    (void)have;
    auto leaf = [&](int slot, R tmax, HitRefT<R>& b) {
        if constexpr (ANY)
            if (found) return false;
        const rt_prim& p = S.leaf_prims[slot];
        const HitRefT<R> before = b;   // (CLOSEST: the closest hit so far, once have)
        bool hit = false, done = false;
        if constexpr ((C::F & FEAT_INST) != 0)
            if (p.kind == RT_PRIM_INSTANCE) {
                hit = instance_t<C>(S, S.instances[p.a], r, t_min, tmax, b, stack, S.blas_base, key, cnt);
                done = true;
            }
        if constexpr ((C::F & FEAT_MEDIUM) != 0)
            if (!done && p.kind == RT_PRIM_MEDIUM) {
                hit = medium_t<C>(S, p, r, t_min, tmax, b.t, stack, S.blas_base, key, cnt);
                done = true;
            }
        if (!done) hit = simple_t<C>(p, r, t_min, tmax, b.t, b.side, cnt, (C::F & FEAT_SHUTTER) != 0);
        if constexpr (ANY) {
            if (hit) {
                found = true;
                b.t = -(R)RT_INF;
            }
        } else {
            // An exact tie (coincident faces: the final scene's ground boxes share their sides; a test
            // rejects t > t_max only, so both accept). hit_hittables' loop keeps the later entry of the
            // list; so does this walk, whatever order its structure tests them in: of two top-level
            // records with the same t the one later in rt_scene_soa.prims stays.
            if (hit && have && b.t == before.t && S.prim_refs[slot] < S.prim_refs[before.prim]) {
                b = before;
                hit = false;
            }
            have = have || hit;
        }
        return hit;
    };
    if (UniformLeaf<C>() && S.tlas_root < 0 && S.tlas_root != RT_DONE) {   // (wave-uniform) a one-leaf top level
        const int code = ~S.tlas_root;
        bool hit = false;
        for (int slot = code >> 5, end = (code >> 5) + (code & 31); slot < end; ++slot) {
            if (leaf(slot, t_max, best)) {   // traverse's do_leaf, in slot order
                best.prim = slot;
                t_max = best.t;
                hit = true;
            }
        }
        return hit;
    }
    return traverse<C, true>(S, S.tlas_root, r, t_min, t_max, best, stack, 0, cnt, leaf);
}

// The geometric primitive of a medium boundary: the boundary prim, through its instance if it has
// one; a boundary that is a BVH has no single primitive behind a medium's t, and the first one down
// its first children stands for the set (rt_abi.h, rt_hit.inner: the one field of a record that
// depends on the acceleration structure).
__device__ __forceinline__ int boundary_prim(const SceneDev& S, int i)
{
    const rt_prim& q = S.prims[i];
    if (q.kind != RT_PRIM_INSTANCE) return i;
    const rt_instance& in = S.instances[q.a];
    if (in.child_kind == RT_CHILD_PRIM) return in.child;
    int ref = in.child;   // a BLAS root: down its first children to a leaf code (slots count from in.pad)
    while (ref >= 0) ref = S.nodes[ref].child[0];
    return S.prim_refs[in.pad + ((~ref) >> 5)];
}

// rt_hit's prim, inner and RT_HIT_MEDIUM of a closest-hit reference: best.prim is the top-level
// leaf slot; best.sub an instance's child prim, or the absolute leaf slot of its BLAS primitive
// (instance_t: the instance's base leaf slot, rt_instance.pad on the device, already added)
template <class C>
__device__ __forceinline__ void hit_ids(const SceneDev& S, const HitRefT<double>& best, int& prim, int& inner, int& flags)
{
    const rt_prim& p = S.leaf_prims[best.prim];
    prim = S.prim_refs[best.prim];
    inner = prim;
    int medium = -1;   // the medium whose record this is
    if constexpr ((C::F & FEAT_INST) != 0) {
        if (p.kind == RT_PRIM_INSTANCE) {
            const rt_instance& in = S.instances[p.a];
            if ((C::F & FEAT_INST_BLAS) == 0 || in.child_kind == RT_CHILD_PRIM) {
                inner = best.sub;
                if constexpr ((C::F & FEAT_INST_MEDIUM) != 0)
                    if (S.prims[inner].kind == RT_PRIM_MEDIUM) medium = inner;
            } else {
                inner = S.prim_refs[best.sub];
            }
        }
    }
    if constexpr ((C::F & FEAT_MEDIUM) != 0)
        if (p.kind == RT_PRIM_MEDIUM) medium = prim;
    if (medium >= 0) {
        flags |= RT_HIT_MEDIUM;
        inner = boundary_prim(S, S.prims[medium].a);
    }
}

// rt_render_features' albedo of a hit record. trace_features (features_device.hpp) holds this
// switch inline in its sample loop, and that header keeps its text (the feature kernels' code is
// pinned), so it is restated here rather than shared.
template <class C>
__device__ __forceinline__ void hit_albedo(const SceneDev& S, const HitT<double>& h, double& cr, double& cg, double& cb)
{
    const rt_material& m = material_of<C>(S, h.mat);
    const int kind = m.kind;
    cr = 1.0; cg = 1.0; cb = 1.0;   // Dielectric: its attenuation
    if (kind == RT_MAT_METAL) {
        cr = m.albedo[0]; cg = m.albedo[1]; cb = m.albedo[2];
    } else if (kind != RT_MAT_DIELECTRIC) {   // Lambertian, Isotropic: the attenuation; DiffuseLight: the emission
        tex_value<C>(S, m.tex, h, cr, cg, cb);
    }
}

typedef double d2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double pack_i32(int lo, int hi)
{
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}
__device__ __forceinline__ bool finite_f64(double x) { return __builtin_fabs(x) < RT_INF; }   // (false for a NaN)

template <class C, int MODE>
__global__ void __launch_bounds__(BlockThreads<C>(), min_waves<C>()) trace_query(SceneDev S, QueryArgs Q)
{
    static_assert(!C::F32 && !C::COUNT, "queries are f64 and do not count work");
    constexpr bool ANY = MODE == RT_QUERY_ANY;
    stage_lds<C>(S);   // every thread of the block takes part, before the tail block's surplus lanes return
    const long long i = (long long)blockIdx.x * BlockThreads<C>() + threadIdx.x;
    if (i >= Q.n) return;
    StackT<C> stack;
    if constexpr (Stack16Cfg<C>()) stack.base = reinterpret_cast<short*>(rt_lds + lds_stack_offset<C>(S)) + threadIdx.x;
    else if constexpr (C::LDS) stack.init((int)lds_stack_offset<C>(S));
    Count cnt{};

    const d2v* q = reinterpret_cast<const d2v*>(Q.rays + i);
    const d2v q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4];
    RayT<double> r;
    r.ox = q0.x; r.oy = q0.y; r.oz = q1.x;
    r.dx = q1.y; r.dy = q2.x; r.dz = q2.y;
    r.time = q3.x;
    const double t_min = q3.y, t_max = q4.x, keys = q4.y;   // keys: key_pixel | key_sample << 32
    const unsigned long long kb = (unsigned long long)__double_as_longlong(keys);

    // rt_abi.h, "Invalid rays"
    bool ok = finite_f64(r.ox) && finite_f64(r.oy) && finite_f64(r.oz) && finite_f64(r.dx) && finite_f64(r.dy) &&
              finite_f64(r.dz) && finite_f64(r.time);
    const double dm = fmax(fmax(__builtin_fabs(r.dx), __builtin_fabs(r.dy)), __builtin_fabs(r.dz));
    ok = ok && dm > 0.0 && t_min <= t_max;   // (the comparison is false when either end is a NaN)
    if (Q.has_moving) ok = ok && r.time >= Q.time_lo && r.time <= Q.time_hi;
    ok = ok && fmax(fmax(__builtin_fabs(r.ox), __builtin_fabs(r.oy)), __builtin_fabs(r.oz)) <= Q.origin_bound;
    if constexpr (C::S32) ok = ok && dm >= 0x1.0p-40 && dm <= 0x1.0p+40;   // f32 slabs hold 1 / d in f32

    HitRefT<double> best;
    HitT<double> h;
    bool hit = false;
    if (ok) {
        finish_ray<C>(r, S.has_spheres != 0);
        const Keyed key{Q.seed, (uint32_t)kb, (uint32_t)(kb >> 32), Q.bounce};
        hit = cast_interval<C, ANY>(S, r, t_min, t_max, best, stack, key, cnt);
    }
    if constexpr (ANY) {
        Q.occluded[i] = hit ? 1 : 0;
    } else {
        double t = ok ? RT_INF : __builtin_nan("");
        double px = 0.0, py = 0.0, pz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, cr = 0.0, cg = 0.0, cb = 0.0;
        int prim = -1, inner = -1, mat = -1, flags = ok ? 0 : RT_HIT_INVALID;
        if (hit) {
            finish_hit<C>(S, r, best, h);
            t = h.t;
            px = h.px; py = h.py; pz = h.pz;
            nx = h.nx; ny = h.ny; nz = h.nz;
            mat = h.mat;
            flags = h.front ? RT_HIT_FRONT : 0;
            hit_ids<C>(S, best, prim, inner, flags);
            if (Q.albedo) hit_albedo<C>(S, h, cr, cg, cb);
        }
        if (Q.hits) {
            d2v* o = reinterpret_cast<d2v*>(Q.hits + i);
            o[0] = d2v{t, px};
            o[1] = d2v{py, pz};
            o[2] = d2v{nx, ny};
            o[3] = d2v{nz, pack_i32(prim, inner)};
            o[4] = d2v{pack_i32(mat, flags), keys};
        }
        if (Q.albedo) {
            double* a = Q.albedo + 3 * (size_t)i;
            a[0] = cr; a[1] = cg; a[2] = cb;
        }
    }
}

// One feature set's kernels (query_v_*.hip instantiate one each): launch_features_variant's choice
// of shape — whole or partial TLAS in LDS, 16-bit stack entries only where they fit and the kernel
// has no static LDS in front of the node records — over one lane per ray.
template <uint32_t F>
hipError_t launch_query_variant(const SceneDev& S, const QueryArgs& Q, int mode, const LaunchOpts& o, hipStream_t stream)
{
    KernelShape k = launch_shape(F, false, S, o);
    if (k.s16) {
        using C16 = Cfg<F, true, true, true, false, false>;
        static const bool static_lds = any_static_lds({(const void*)trace_query<C16, RT_QUERY_CLOSEST>,
                                                       (const void*)trace_query<C16, RT_QUERY_ANY>});
        if (static_lds) k = without_stack16(k);
    }
    const int bt = k.block_threads;
    const size_t lds = launch_lds_bytes(k, S);
    const unsigned nb = (unsigned)((Q.n + bt - 1) / bt);
    with_cfg<F, false, false>(k, [&](auto whole, auto part) {
        using W = decltype(whole);
        using P = decltype(part);
        const auto kernel = mode == RT_QUERY_ANY ? (k.nall ? trace_query<W, RT_QUERY_ANY> : trace_query<P, RT_QUERY_ANY>)
                                                 : (k.nall ? trace_query<W, RT_QUERY_CLOSEST> : trace_query<P, RT_QUERY_CLOSEST>);
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(bt), lds, stream, S, Q);
    });
    return hipGetLastError();
}
#define RT_QUERY_DECL(F) \
    extern template hipError_t launch_query_variant<F>(const SceneDev&, const QueryArgs&, int, const LaunchOpts&, hipStream_t);
RT_QUERY_DECL(FEAT_SET_SPHERES)
RT_QUERY_DECL(FEAT_SET_RECTINST)
RT_QUERY_DECL(FEAT_SET_MEDIA)
RT_QUERY_DECL(FEAT_SET_FINAL)
RT_QUERY_DECL(FEAT_ALL)
#undef RT_QUERY_DECL

}  // namespace rtk
