// denoise_core.hpp — the arithmetic of the variance-guided NL-means filter (include/rt/rt_abi.h,
// rt_denoise), one definition for the device kernel (denoise_kernel.hip) and the host filter
// (denoise_host.cpp): the point distance, the weight, the finite-value rules, the number of
// valid patch terms, and rt_denoise_guided's feature term. Compiled without contraction and without fast math, so both sides do the
// same f64 operations in the same order. Compiles without HIP: denoise_host.cpp is plain C++.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RT_DN_HD __host__ __device__
#else
#define RT_DN_HD
#endif

#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace rtk {

constexpr int kDenoiseMaxRadius = 10;
constexpr int kDenoiseMaxPatch = 3;

// adaptive_luma's expression (adaptive_criterion.hpp): Rec. 709 luminance, left to right
RT_DN_HD inline double denoise_luma(double r, double g, double b)
{
    return 0.2126 * r + 0.7152 * g + 0.0722 * b;
}

// false for NaN and +-Inf
RT_DN_HD inline bool denoise_finite(double x)
{
    return x - x == 0.0;
}

// delta(a, o) from Y and V = se^2 of a and of b = a + o; k2 = k * k. Not symmetric in (a, b).
RT_DN_HD inline double denoise_delta(double ya, double va, double yb, double vb, double k2)
{
    const double d = ya - yb;
    const double vmin = va < vb ? va : vb;
    return (d * d - (va + vmin)) / (1e-10 + k2 * (va + vb));
}

// w from the patch distance D: exp(-max(0, D)), 0 when D is not finite
RT_DN_HD inline double denoise_weight(double D)
{
    if (!denoise_finite(D)) return 0.0;
    return ::exp(-(D > 0.0 ? D : 0.0));
}

// ---- feature guides (rt_denoise_guided): the weight's second term, per pixel pair ----------------
// The guide frames of a call and the reciprocals of their squared sigmas (1 / (sigma * sigma),
// computed once on the host in f64); a null frame's term is skipped.
struct DenoiseGuides {
    const double* albedo = nullptr;   // height x width x 3
    const double* normal = nullptr;   // height x width x 3
    const double* depth = nullptr;    // height x width
    double ia = 0.0, in = 0.0, iz = 0.0;
    RT_DN_HD bool any() const { return albedo || normal || depth; }
};

// squared distance of a 3-channel feature between pixels p and q: (a0 a0 + a1 a1) + a2 a2
RT_DN_HD inline double denoise_feature_dist3(const double* f, size_t p, size_t q)
{
    const double a0 = f[3 * p + 0] - f[3 * q + 0];
    const double a1 = f[3 * p + 1] - f[3 * q + 1];
    const double a2 = f[3 * p + 2] - f[3 * q + 2];
    return (a0 * a0 + a1 * a1) + a2 * a2;
}

// the depth term: relative, so one sigma serves near and far surfaces
RT_DN_HD inline double denoise_depth_dist(double zp, double zq)
{
    const double z = zp - zq;
    return z * z / (1e-10 + (zp * zp + zq * zq));
}

// Phi(p, o) for q = p + o: dA * ia + dN * in + dZ * iz, left to right over the guides present
RT_DN_HD inline double denoise_phi(const DenoiseGuides& g, size_t p, size_t q)
{
    double phi = 0.0;
    if (g.albedo) phi = phi + denoise_feature_dist3(g.albedo, p, q) * g.ia;
    if (g.normal) phi = phi + denoise_feature_dist3(g.normal, p, q) * g.in;
    if (g.depth) phi = phi + denoise_depth_dist(g.depth[p], g.depth[q]) * g.iz;
    return phi;
}

// w from the patch distance D and the feature term: exp(-(max(0, D) + Phi)), 0 when either is
// not finite
RT_DN_HD inline double denoise_weight_guided(double D, double phi)
{
    if (!denoise_finite(D) || !denoise_finite(phi)) return 0.0;
    return ::exp(-((D > 0.0 ? D : 0.0) + phi));
}

// Along one axis of an n-pixel image: the number of s in [-f, f] with p + s and p + s + d both in
// [0, n). At least 1 when p and p + d are.
RT_DN_HD inline int denoise_axis_count(int p, int d, int f, int n)
{
    int lo = p - f, hi = p + f;
    const int lo_min = d < 0 ? -d : 0, hi_max = d > 0 ? n - 1 - d : n - 1;
    lo = lo > lo_min ? lo : lo_min;
    hi = hi < hi_max ? hi : hi_max;
    return hi - lo + 1;
}

}  // namespace rtk
