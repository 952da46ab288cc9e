// denoise_core.hpp — the arithmetic of the variance-guided NL-means filter (include/rt/rt_abi.h,
// rt_denoise), one definition for the device kernel (denoise_kernel.hip) and the host filter
// (denoise_host.cpp): the point distance, the weight, the finite-value rules and the number of
// valid patch terms. Compiled without contraction and without fast math, so both sides do the
// same f64 operations in the same order. Compiles without HIP: denoise_host.cpp is plain C++.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RT_DN_HD __host__ __device__
#else
#define RT_DN_HD
#endif

#include <math.h>
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
