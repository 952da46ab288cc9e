// root_bracket.hpp — f32 brackets of a sphere test's f64 roots, and the closest-hit decision taken
// from them (RT_OPT_DEFER_ROOTS; trace_pool's CfgDefer instantiations).
//
// sphere_t (trace_prims.hpp) computes, for a candidate with disc >= 0,
//     near = RN(RN(-half_b - RN(sqrt(disc))) / a),   far = RN(RN(-half_b + RN(sqrt(disc))) / a)
// (div_rcp gives the division's bits), an f64 square root and one or two quotients per candidate. A
// cast needs those bits for its closest sphere only; for every other candidate it needs three
// decisions — near or far root against t_min, in range or not, closer than the best so far or not —
// and an f32 estimate with a proven error bound decides them almost always.
//
// The bound. With H = half_b, s = sqrt(disc), and
//     hbf = (float)H, sf = sqrt32((float)disc), yaf = (float)ya      (ya = RN(1 / a), as RayT::ya)
//     t32 = RN32(RN32(-hbf -+ sf) * yaf),   E = RN32(RN32(RN32(|hbf| + sf) * yaf) * 2^-21)
// every computed f64 root lies in [RN32(t32 - E), RN32(t32 + E)], given the premises below. With
// u = 2^-24 (half an f32 ulp, relative), U = (|H| + s) / a and T = (-H -+ s) / a the real root:
//   - |hbf - H| <= u |H|;  (float)disc = disc (1 + d), |d| <= u, and sqrt32 is within one ulp
//     (v_sqrt_f32's accuracy; the host's sqrtf is within half), so |sf - s| <= (u / 2 + 2 u + ...) s
//     < 2.6 u s;  together |(-hbf -+ sf) - (-H -+ s)| < 2.6 u (|H| + s);
//   - the f32 sum rounds by at most u |-hbf -+ sf| <= u (1 + 2.6 u)(|H| + s): 3.6 u (|H| + s) so far,
//     with the higher-order terms 3.7 u;
//   - yaf = (1 / a)(1 + e), |e| <= u + 2^-53, and the product rounds by u once more: each at most
//     u (1 + 4 u) U, so |t32 - T| < (3.7 + 2.1) u U = 5.8 u U;
//   - the f64 root differs from T by at most 3 x 2^-53 U (the root, the sum and the quotient round once
//     each): below 0.01 u U;
//   - E >= 8 u U (1 - 4 u) (three f32 roundings and the two conversions, each against it), and the
//     final t32 -+ E rounds by at most u (|t32| + E) <= 1.01 u U.
// 5.8 + 0.01 + 1.01 = 6.82 < 8 (1 - 4 u): the bracket holds with a sixth to spare, and strictly (the
// root is never an end point), which the walk's pruning by `hi` relies on for ties.
// Premises: (float)disc >= 2^-80, yaf in [2^-60, 2^60], and no f32 overflow. Then nothing above loses
// bits to f32 underflow: sf >= 2^-40, U >= 2^-100, E >= 2^-122 is a normal number, and where t32
// itself comes out subnormal (after cancellation) its rounding error, at most 2^-150, is far inside
// E. A tiny or zero H needs no premise: its conversion error is at most 2^-150, against 2.6 u s >=
// 2^-62. Outside them the brackets decide nothing, by construction rather than by a test of each
// premise: `ya32` turns a yaf outside its range into NaN and `roots` does the same to sf, which
// makes all four ends NaN; and an overflow anywhere makes E infinite or NaN (|t32| <= E 2^21, so
// E is the first to go), which leaves every lower end -inf or NaN and every upper end +inf or NaN.
// NaN or infinite inputs, disc == 0, and ya = NaN (|d|^2 outside div_rcp's guard) all end there:
// every comparison below is true only for ordered, finite ends on the deciding side, so such a
// bracket falls to "ambiguous", never to a decision.
//
// No HIP: the kernel (trace_walk.hpp), the host twin and tests/root_bracket_main.cpp run the same
// `closer`.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RT_RB_HD __host__ __device__ inline
#else
#define RT_RB_HD inline
#endif

namespace rtrb {

// f32 bounds of a double, rounded outward (trace_prims.hpp's f32_down / f32_up: the same values)
RT_RB_HD float down(double t)
{
    const float f = (float)t;
    return f > 0.0f ? f * (1.0f - 0x1.0p-20f) : f * (1.0f + 0x1.0p-20f);
}
RT_RB_HD float up(double t)
{
    const float f = (float)t;
    return f > 0.0f ? f * (1.0f + 0x1.0p-20f) : f * (1.0f - 0x1.0p-20f);
}

// an f32 square root within one ulp (the device's bare v_sqrt_f32: no correction sequence)
RT_RB_HD float sqrt32(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return __builtin_sqrtf(x);
#endif
}

// The ray's part, once per cast: yaf from RayT::ya = RN(1 / |d|^2) (NaN outside div_rcp's guard),
// NaN outside the bound's range.
RT_RB_HD float ya32(double ya)
{
    const float y = (float)ya;
    return y >= 0x1.0p-60f && y <= 0x1.0p+60f ? y : __builtin_nanf("");
}

// The brackets [nlo, nhi] of sphere_t's near root and [flo, fhi] of its far root, from the f64 values
// the exact path has: half_b and disc >= 0, and the ray's ya32. false: outside the bound's premises
// — the brackets decide nothing (above).
RT_RB_HD bool roots(double half_b, double disc, float yaf, float& nlo, float& nhi, float& flo, float& fhi)
{
    const float hbf = (float)half_b, df = (float)disc;
    const float sf = df >= 0x1.0p-80f ? sqrt32(df) : __builtin_nanf("");
    const float e = ((__builtin_fabsf(hbf) + sf) * yaf) * 0x1.0p-21f;
    const float tn = (-hbf - sf) * yaf, tf = (sf - hbf) * yaf;
    nlo = tn - e;
    nhi = tn + e;
    flo = tf - e;
    fhi = tf + e;
    return e < __builtin_inff();
}

// What a walk keeps of its closest hit so far: the leaf slot and a bracket of its exact t.
// prim < 0: none yet, lo = hi = +inf.
struct Best {
    int prim;
    float lo, hi;
};
RT_RB_HD Best none() { return Best{-1, __builtin_inff(), __builtin_inff()}; }

// how often `closer` decided from brackets and how often it took the exact path (the host twin)
struct Tally {
    long long bracket = 0, exact = 0;
};

// One candidate (leaf slot `slot`, its half_b and disc >= 0 — or NaN, which sphere_t lets through —
// against the best so far, as sphere_t with t_max = the best's exact t decides it: accepted with
// its near root if that is >= t_min, else its far root if that is, and only if !(t_max < root), so
// a root equal to the best's wins (the later-tested sphere takes a tie). [tmin_lo, tmin_hi] is an
// f32 bracket of t_min. From brackets:
//     near lo >= t_min -> the near root;  near hi < t_min -> the far root, decided the same way
//     (far hi < t_min: no hit);  lo > best.hi -> farther (even before the root is chosen: both are
//     at least lo);  hi < best.lo -> closer;
// anything else, equality included, is ambiguous and decided exactly: exact_self(t) is this
// candidate's sphere_t over [t_min, +inf), exact_of(slot, t) the same for the best's slot. The
// winner of an exact decision keeps the outward-rounded f32 bounds of its t. true: `best` is now
// this candidate.
template <class ExactSelf, class ExactOf>
RT_RB_HD bool closer(Best& best, int slot, double half_b, double disc, float yaf, float tmin_lo, float tmin_hi,
                     ExactSelf&& exact_self, ExactOf&& exact_of, Tally* tally = nullptr)
{
    float nlo, nhi, flo, fhi;
    (void)roots(half_b, disc, yaf, nlo, nhi, flo, fhi);
    // Straight-line up to the rare exact path: a wave runs this at every leaf step. The candidate's
    // root, if it has one in range, is the far root when the near one is surely below t_min, else
    // the near or the far one — at least `lo` either way (far >= near).
    const bool use_far = nhi < tmin_lo;
    const float lo = use_far ? flo : nlo, hi = use_far ? fhi : nhi;
    const bool behind = fhi < tmin_lo;                     // both roots below t_min: no hit
    const bool farther = lo > best.hi;                     // whichever root it is, the best is closer
    const bool sure = lo >= tmin_hi && hi < best.lo;       // this root, in range, and closer
    best.prim = sure ? slot : best.prim;
    best.lo = sure ? lo : best.lo;
    best.hi = sure ? hi : best.hi;
    if (__builtin_expect(behind || farther || sure, 1)) {
        if (tally) tally->bracket++;
        return sure;
    }
    if (tally) tally->exact++;
    double t;
    if (!exact_self(t)) return false;
    double tb = (double)__builtin_inff();
    if (best.prim >= 0) (void)exact_of(best.prim, tb);
    if (tb < t) {   // sphere_t's `t_max < root`
        best.lo = down(tb);
        best.hi = up(tb);
        return false;
    }
    best.prim = slot;
    best.lo = down(t);
    best.hi = up(t);
    return true;
}

}  // namespace rtrb
