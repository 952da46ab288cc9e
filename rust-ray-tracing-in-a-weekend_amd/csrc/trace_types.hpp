// trace_types.hpp — the megakernel's types and arithmetic (first layer of trace_device.hpp, which
// holds the execution model): rays, hit records, the work counters, the compile-time configuration
// (Cfg and the reduced configurations of nested code), the traversal stack, division through a
// correctly rounded reciprocal, the precision-generic r_* helpers and finish_ray.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "rt/rt_numerics.h"
#include "rt/rt_scene.h"
#include "trace_kernel.hpp"

namespace rtk {

// R: the path's arithmetic type — double (the reference's f64, math.rs:13-17; path-identical
// to the oracle: the same rays, hits and draws, per-pixel means within last-ulp summation
// differences) or float (the f32 fast mode; statistically equal).
typedef float f2v __attribute__((ext_vector_type(2)));
template <class R>
struct RayT {
    R ox, oy, oz;
    R dx, dy, dz;
    R time;
    R a;                      // length_squared(direction)
    R ya;                     // f64: 1 / a correctly rounded (NaN outside [2^-900, 2^900]: see div_rcp)
    R ix, iy, iz;             // 1 / direction (f64 slab tests only)
    R yx, yy, yz;             // f64, scenes with rects: RN(1 / direction) for div_rcp (NaN outside its range)
    // f32 slab terms per axis (f32 slab tests only): (1 / direction, -origin * (1 / direction)),
    // a register pair each, so one v_pk_fma_f32 takes both for the two children of a node
    // (op_sel: the pair's low half as the factor, its high half as the addend, in both lanes)
    f2v sx, sy, sz;
    uint32_t onx, ony, onz;   // byte offsets in a node of child 0's near planes (by direction sign)
};

// The HitRecord of hittable.rs:6-27 (uv deferred to texture lookup: uvkind 1 keeps the
// object-space outward normal for sphere_uv, 2 keeps (x-a0, a1-a0, y-b0, b1-b0)).
template <class R>
struct HitT {
    R t, px, py, pz, nx, ny, nz;
    R uv0, uv1, uv2, uv3;
    int front, mat, uvkind;
};
using Hit = HitT<double>;

// What traversal keeps per candidate: the parameter and which primitive produced it.
template <class R>
struct HitRefT {
    R t;
    int prim;   // prim index (top level)
    int sub;    // instance: BLAS prim index; box: winning side (0..5)
    int side;   // box inside an instance: winning side
};

struct Keyed {                 // coordinates of the medium's keyed draw
    uint64_t seed;
    uint32_t pixel, sample, bounce;
};

struct Count {
    uint32_t casts, nodes, prims;
    uint32_t wave_steps, wave_nodes;  // loop iterations the wave executed (counted by its first active lane)
    uint32_t wave_leaves;             // leaf-loop iterations the wave executed
    uint32_t cam_lanes, cam_steps;    // lanes starting a sample / iterations in which any did
    uint32_t shade_lanes, shade_steps;
    uint64_t t_nodes, t_leaves;       // wave-cycles in node-visit loops / leaf tests (same in every lane)
    // pool kernels, finer phases (wave-cycles; each added by the first active lane of the region
    // it times, so summed over lanes they are wave totals): ray set-up, the walk's prologue
    // (pre-leaf test, bounds), the hit record, and inside the leaf tests the media and instances
    uint64_t t_setup, t_pre, t_rec, t_med, t_inst, t_refill, t_defer;
    // ray generation split (pool kernels): path seeding + camera jitter, the rejection loop
    uint64_t t_seed, t_tries;
    // pool kernels, why a lane of a bounce-loop iteration casts no ray (with casts they add up to
    // 64 x wave_steps): no unit left to take (the launch's tail), every ring slot holding an
    // unfinished block (RING), a path that ended in its scatter (the material absorbed it), the
    // depth cap, a rejection loop left for the next iteration (RT_TRY_LEFT)
    uint32_t idle_tail, idle_ring, no_scatter, depth_cap, try_wait;
};
// COUNT phase stamps: tp is the lane's last stamp; the first active lane adds the interval
#define RT_STAMP(acc, tp)                                                   \
    do {                                                                    \
        if (C::COUNT) {                                                     \
            const uint64_t t_ = __builtin_amdgcn_s_memtime();               \
            if (first_active_lane()) (acc) += t_ - (tp);                    \
            (tp) = t_;                                                      \
        }                                                                   \
    } while (0)
// COUNT only: true in exactly one active lane of the wave
__device__ __forceinline__ bool first_active_lane()
{
    return (int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1;
}

// Compile-time kernel configuration (one instantiation per variant):
//   F      scene features the variant handles (trace_kernel.hpp FEAT_*); code for the
//          others is not emitted, which keeps register pressure and code size down
//   S32    conservative f32 slab tests (boxes padded on the host, see flatten.cpp)
//   LDS    traversal stack in LDS (interleaved per lane) instead of scratch
//   COUNT  diagnostic: count casts / node visits / primitive tests and time the phases
// Traversal is while-while (Aila & Laine 2009); the if-if form, speculative while-while and
// a per-lane state machine with ballot-gated shading all measured slower (DESIGN.md §5.2;
// the rejected experiments are kept as patches under scripts/experiments/).
//   NALL   every TLAS node is in LDS (no per-node LDS/global choice)
#ifndef RT_TRY_LEFT
// pool schedules: the wave leaves its rejection loop (random_in_unit_disk /
// random_in_unit_sphere tries, math.rs:51-76) once at most RT_TRY_LEFT lanes still reject, after
// at least RT_TRY_MIN tries; those lanes keep their stream position and candidate state and go
// on drawing in the next bounce-loop iteration instead of tracing in this one. Each lane's draws
// stay in its own stream order, so the bits do not change; the wave no longer runs as many
// tries as its unluckiest lane (E[max of 64 geometric(0.52)] ~ 6.9 against a mean of 1.9).
// 0: the loop runs until every lane accepted (round 3). C2 1200x800x100 (profiles/r04b_ab_c2.log):
// off 15.28 ms, 2 15.12, 4 15.07, 8 15.37, 4 after one try 15.22; images identical.
#define RT_TRY_LEFT 4
#endif
#ifndef RT_TRY_MIN
#define RT_TRY_MIN 2
#endif
// the variants the cap applies to: the spheres ones (C2, C5) and the Cornell box's (C3 800x800x200
// 46.00 -> 45.80 ms, profiles/r04d_ab_c3.log). The final scene's is 1-2 % slower with it (C4
// 1920x1080x100 106.84 -> 109.04 ms, r04c_ab_c4.log; 107.83 -> 109.19, r04d_ab_c4.log): its
// iterations are long, so a lane that sits one out loses more than the wave saves on tries
template <class C>
constexpr bool TryLeft() { return RT_TRY_LEFT > 0 && (C::F == FEAT_SET_SPHERES || C::F == FEAT_SET_RECTINST); }
//   F32    the f32 fast mode (Real = float): statistically, not bitwise, equal
template <uint32_t F_, bool S32_, bool LDS_, bool NALL_, bool COUNT_, bool F32_ = false>
struct Cfg {
    static constexpr uint32_t F = F_;
    static constexpr bool S32 = S32_;
    static constexpr bool LDS = LDS_;
    static constexpr bool NALL = NALL_;
    static constexpr bool COUNT = COUNT_;
    static constexpr bool F32 = F32_;
    // what the instantiation launches as (launch_shapes.hpp): a property of the launched kernel,
    // inherited by the reduced configurations of nested code (CfgDrop), which share its LDS
    static constexpr KernelShape SHAPE = kernel_shape(F_, S32_, LDS_, NALL_, F32_);
    static_assert(SHAPE.s32 == S32_ && SHAPE.lds == LDS_ && SHAPE.nall == NALL_ && SHAPE.f32 == F32_, "the shape of this Cfg");
    using Real = typename std::conditional<F32_, float, double>::type;
    static constexpr bool STAGE = false;   // (CfgStage below)
    static constexpr bool PRIMARY = false; // (CfgPrimary below)
    static constexpr bool DEFER = false;   // (CfgDefer below)
};
// The configuration of trace_pool's staged instantiations (launch_shapes.hpp, RT_STAGE_SEEDS): the
// wave seeds and jitters a whole row of samples at once. A configuration of its own rather than a
// template parameter of the kernel, so every other instantiation keeps its symbol and its code.
template <class C>
struct CfgStage : C {
    static constexpr bool STAGE = true;
};

// The staged per-sample pool kernel whose new samples take their first hit from their pixel's
// candidate list (primary_candidates.hpp, KParams.primary; trace_pool.hpp) instead of a walk: the f64
// spheres variant's timed kernels only. A wrapper like CfgStage, for the same reason.
template <class C>
struct CfgPrimary : CfgStage<C> {
    static constexpr bool PRIMARY = true;
};

// The primary-candidate kernel whose sphere tests decide from f32 brackets of the roots and compute
// the exact root of a cast's winner only (root_bracket.hpp, RT_OPT_DEFER_ROOTS; trace_walk.hpp,
// trace_world_defer). A wrapper once more: the CfgPrimary kernels keep their symbols and their code.
template <class C>
struct CfgDefer : CfgPrimary<C> {
    static constexpr bool DEFER = true;
};

// The configuration of code reached only through an instance or a medium boundary: the
// feature bits the scene does not need there are dropped (FEAT_INST_RECT / FEAT_MEDIUM_INST
// clear), so e.g. the final scene's instanced BLAS of spheres compiles the sphere test only.
// threads per workgroup (RT_BLOCK_FINAL; the LDS stack's lane stride)
template <class C>
constexpr int BlockThreads() { return C::SHAPE.block_threads; }

template <class C, uint32_t DROP>
struct CfgDrop : C {
    static constexpr uint32_t F = C::F & ~DROP;
};
// Spheres reached only through an instance or a medium boundary are static unless the scene
// says otherwise (FEAT_NEST_MOVING): their test then loads no velocity (FEAT_STATIC; the final
// scene's instanced cluster and its fog / glass-medium boundaries), which shortens the nested
// walk's live ranges; c0 + 0 * s is c0 bit for bit, so the result is the same.
template <class C, uint32_t DROP>
struct CfgDropStatic : C {
    static constexpr uint32_t F = (C::F & ~DROP) | ((C::F & FEAT_NEST_MOVING) ? 0u : (uint32_t)FEAT_STATIC);
};
template <class C>
using InstC = CfgDropStatic<C, (C::F & FEAT_INST_RECT) ? 0u : (uint32_t)FEAT_RECT>;
template <class C>
using BoundC = CfgDropStatic<C, FEAT_INST_MEDIUM | ((C::F & FEAT_MEDIUM_INST) ? 0u : (uint32_t)(FEAT_RECT | FEAT_INST))>;
template <class C>
using InstMedC = CfgDropStatic<C, FEAT_INST_MEDIUM>;   // a medium under an instance: no medium below it

// Traversal stack. LDS: a lane-interleaved dynamic LDS array [entry][block threads]
// (consecutive lanes hit consecutive banks) sized per scene by the host (TLAS depth +
// BLAS depth); scratch: a private array (deep scenes).
extern __shared__ int rt_lds[];  // [cached TLAS nodes] [stack entries x block lanes] [materials, textures]
// The lane's index in its wave, recomputed where it is used (volatile: not CSE'd into one
// value that stays live through the bounce loop; at 128 VGPRs the final variant spilled the
// stack base it replaces and reloaded it from scratch at every walk)
__device__ __forceinline__ int lane_remat()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
template <bool LDS, bool REMAT = false, int BT = 256>
struct Stack;
template <int BT>
struct Stack<true, true, BT> {   // the variants with nested walks (128 VGPRs)
    int wave0;   // rt_lds index of this wave's lane 0, entry 0 (wave-uniform: an SGPR)
    __device__ __forceinline__ int& operator[](int i) const { return rt_lds[wave0 + lane_remat() + i * BT]; }
    __device__ __forceinline__ void init(int stack_off)
    {
        wave0 = stack_off + __builtin_amdgcn_readfirstlane((int)threadIdx.x & ~63);
    }
};
template <int BT>
struct Stack<true, false, BT> {   // (Cornell variants: the remat costs 0.3-0.9 %, nothing spills)
    int* base;
    __device__ __forceinline__ int& operator[](int i) const { return base[i * BT]; }
    __device__ __forceinline__ void init(int stack_off) { base = rt_lds + stack_off + threadIdx.x; }
};
template <int BT>
struct Stack<false, false, BT> {
    int v[66];   // 32 + 32 entries + the two walks' RT_DONE sentinels
    __device__ __forceinline__ int& operator[](int i) { return v[i]; }
};
template <int BT>
struct Stack16 {   // node records at LDS addresses < 32 KB, leaf codes > -32768 (SceneDev.stack16_ok)
    short* base;
    __device__ __forceinline__ short& operator[](int i) const { return base[i * BT]; }
};
template <class C>
constexpr bool Stack16Cfg() { return C::SHAPE.s16; }   // (launch_shapes.hpp, RT_STACK16)
template <class C>
using StackT = typename std::conditional<Stack16Cfg<C>(), Stack16<BlockThreads<C>()>,
                                         Stack<C::LDS, C::LDS && (C::F & FEAT_INST_BLAS) != 0, BlockThreads<C>()>>::type;

// Division by a value b used many times, through its correctly rounded reciprocal
// y = RN(1/b): q0 = RN(q*y), then one correction q1 = RN(q0 + RN-exact(q - b*q0) * y).
// With y correctly rounded this is Markstein's theorem (IBM J. R&D 34(1), 1990): q1 =
// RN(q/b), bit for bit what `q / b` gives, barring overflow / underflow in the products,
// which the range guard on b excludes (y is NaN outside it, and the division runs then);
// checked on 8e8 random and adversarial pairs on the host (all-ones / power-of-two
// significands, both signs, exponents -20..20). A zero q may come out as -0 where q / b
// gives +0 or the reverse; every caller compares the quotient with t_min > 0 first or
// has q, b >= 0, so the sign of a zero quotient changes nothing.
__device__ __forceinline__ double rcp_for_div(double b)
{
    const double m = __builtin_fabs(b);
    return (m >= 0x1.0p-900 && m <= 0x1.0p+900) ? 1.0 / b : __builtin_nan("");
}
__device__ __forceinline__ double div_rcp(double q, double b, double y)
{
    const double q0 = q * y;
    const double q1 = __builtin_fma(__builtin_fma(-b, q0, q), y, q0);
    if (__builtin_expect(q1 != q1, 0)) return q / b;  // y outside the guard (or q not finite)
    return q1;
}

__device__ __forceinline__ float f32_inv_dir(double d)
{
    // an exact 0 would give inf * 0 = NaN in the slab products; a 1e-30 component keeps the
    // interval of a ray parallel to a slab finite and correct (inside: huge, outside: empty)
    float f = (float)d;
    if (__builtin_fabsf(f) < 1e-30f) f = __builtin_copysignf(1e-30f, f);
    return __builtin_amdgcn_rcpf(f);
}

// ---- precision-generic helpers: double = the reference's libm restated (rt_numerics.h,
// bit-identical host/device), float = the device's f32 functions (f32 mode only)
__device__ __forceinline__ double r_sqrt(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float r_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double r_fabs(double x) { return __builtin_fabs(x); }
__device__ __forceinline__ float r_fabs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double r_floor(double x) { return __builtin_floor(x); }
__device__ __forceinline__ float r_floor(float x) { return __builtin_floorf(x); }
__device__ __forceinline__ double r_fmin(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float r_fmin(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ double r_sin(double x) { return rt_sin(x); }
__device__ __forceinline__ float r_sin(float x) { return sinf(x); }
__device__ __forceinline__ double r_log(double x) { return rt_log(x); }
__device__ __forceinline__ float r_log(float x) { return logf(x); }
__device__ __forceinline__ double r_acos(double x) { return rt_acos(x); }
__device__ __forceinline__ float r_acos(float x) { return acosf(x); }
__device__ __forceinline__ double r_atan2(double y, double x) { return rt_atan2(y, x); }
__device__ __forceinline__ float r_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double r_pow5(double x) { return rt_pow5(x); }
__device__ __forceinline__ float r_pow5(float x) { const float x2 = x * x; return x2 * x2 * x; }
template <class R>
__device__ __forceinline__ int32_t r_sat_i32(R x) { return rt_sat_i32((double)x); }
template <class R>
__device__ __forceinline__ uint64_t r_sat_u64(R x) { return rt_sat_u64((double)x); }

// Rect / box tests divide through the ray's correctly rounded reciprocals (div_rcp, same
// bits, 3 FMAs instead of an f64 division per face): in the rects + instances variant only —
// the media and final-scene variants would spill the 6 VGPRs the reciprocals hold. Round 3,
// without machine LICM, Cornell 800x800x200 45.76 vs 47.04 ms (r03d_ab_c3.log); round 2 measured
// it slower (58.1 vs 56.5) when its registers spilled.
template <class C>
constexpr bool RectRcp()
{
    return !C::F32 && (C::F & FEAT_RECT) != 0 && (C::F & (FEAT_MEDIUM | FEAT_NOISE | FEAT_IMAGE)) == 0;
}

// A Box's six sides through three per-box reciprocals (box_t): in the variants with Perlin or
// image textures (final scene: 80.0 -> 78.6 ms), whose 3 waves per SIMD the extra live values do
// not change; the 4-wave Cornell variant spills them (49.6 -> 51.6 ms) and Cornell smoke's
// media variant loses too (39.1 -> 39.5; profiles/r02_ab_boxrcp_*.log)
template <class C>
constexpr bool BoxRcp()
{
    return !C::F32 && (C::F & (FEAT_NOISE | FEAT_IMAGE)) != 0;
}

// spheres: the scene has spheres (wave-uniform); otherwise no root division needs 1/a.
// SLABS = false: no node-slab terms (a ray that meets one primitive, e.g. an instance's child)
template <class C, bool SLABS = true>
__device__ __forceinline__ void finish_ray(RayT<typename C::Real>& r, bool spheres)
{
    r.a = r.dx * r.dx + r.dy * r.dy + r.dz * r.dz;
    if constexpr (!C::F32) r.ya = (C::F == FEAT_SET_SPHERES || spheres) ? rcp_for_div(r.a) : __builtin_nan("");
    if constexpr (RectRcp<C>()) {
        r.yx = rcp_for_div(r.dx);
        r.yy = rcp_for_div(r.dy);
        r.yz = rcp_for_div(r.dz);
    }
    if constexpr (!SLABS) {
    } else if constexpr (C::S32) {
        r.sx.x = f32_inv_dir(r.dx);
        r.sy.x = f32_inv_dir(r.dy);
        r.sz.x = f32_inv_dir(r.dz);
        r.sx.y = -(float)r.ox * r.sx.x;
        r.sy.y = -(float)r.oy * r.sy.x;
        r.sz.y = -(float)r.oz * r.sz.x;
        // the LDS node (LdsNode): per axis [lo0 lo1 hi0 hi1 lo0 lo1] at bytes 0/24/48; the
        // near planes of both children at +0 (direction >= 0) or +8, the far ones 8 bytes on
        r.onx = r.sx.x >= 0.0f ? 0u : 8u;
        r.ony = r.sy.x >= 0.0f ? 24u : 32u;
        r.onz = r.sz.x >= 0.0f ? 48u : 56u;
    } else {
        r.ix = (typename C::Real)1 / r.dx;
        r.iy = (typename C::Real)1 / r.dy;
        r.iz = (typename C::Real)1 / r.dz;
    }
}

// hittable.rs:23-26
template <class R>
__device__ __forceinline__ void set_face_normal(HitT<R>& h, R dx, R dy, R dz, R nx, R ny, R nz)
{
    const bool front = dx * nx + dy * ny + dz * nz < (R)0;
    h.front = front;
    h.nx = front ? nx : -nx;
    h.ny = front ? ny : -ny;
    h.nz = front ? nz : -nz;
}

}  // namespace rtk
