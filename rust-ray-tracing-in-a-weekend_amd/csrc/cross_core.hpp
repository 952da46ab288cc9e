// cross_core.hpp — what the cross-filtered NL-means (include/rt/rt_abi.h, rt_denoise_cross) adds to
// denoise_core.hpp's arithmetic, one definition for the device kernels (cross_kernel.hip) and the
// host filter (cross_host.cpp): the staged Y_A, Y_B and V of a pixel with the bad-pixel rule, the
// half difference e(p), and stderr_out's 3 x 3 rule over it (atrous_core.hpp's Vbar rule). The point
// distance, the weights, the patch counts and the feature term are denoise_core.hpp's. Compiled
// without contraction and without fast math, so both sides do the same f64 operations in the same
// order. Compiles without HIP: cross_host.cpp is plain C++.
#pragma once

#include "atrous_core.hpp"
#include "denoise_core.hpp"

namespace rtk {

// Y_A, Y_B and V = scale (se se) of one pixel from its two half means and its standard error. A bad
// pixel (one of the three not finite) gets NaN for both Y, so no pair that touches it has a weight.
struct CrossCell {
    double ya, yb, v;
};

RT_DN_HD inline CrossCell cross_cell(double a0, double a1, double a2, double b0, double b1, double b2, double se,
                                     double scale)
{
    CrossCell c;
    c.ya = denoise_luma(a0, a1, a2);
    c.yb = denoise_luma(b0, b1, b2);
    c.v = scale * (se * se);
    if (!denoise_finite(c.ya) || !denoise_finite(c.yb) || !denoise_finite(c.v)) c.ya = c.yb = (double)NAN;
    return c;
}

// whether a staged cell is a bad pixel's (cross_cell gave it NaN)
RT_DN_HD inline bool cross_bad(double ya)
{
    return !denoise_finite(ya);
}

// e(p) = 0.5 (Y(F_A(p)) - Y(F_B(p)))
RT_DN_HD inline double cross_half_diff(const double fa[3], const double fb[3])
{
    return 0.5 * (denoise_luma(fa[0], fa[1], fa[2]) - denoise_luma(fb[0], fb[1], fb[2]));
}

// E2 = e e over a frame of e, as atrous_vbar reads a variance
struct CrossE2 {
    const double* e;
    int W;
    RT_DN_HD double var(int x, int y) const
    {
        const double v = e[(size_t)y * (size_t)W + (size_t)x];
        return v * v;
    }
};

// stderr_out(p): sqrt of the 3 x 3 binomial mean of E2 around p (the Vbar rule); where E2(p) itself
// is not finite, sqrt(E2(p))
RT_DN_HD inline double cross_stderr(const double* e, int x, int y, int W, int H)
{
    const CrossE2 acc{e, W};
    const double e2 = acc.var(x, y);
    if (!denoise_finite(e2)) return ::sqrt(e2);
    return ::sqrt(atrous_vbar(acc, x, y, W, H));
}

}  // namespace rtk
