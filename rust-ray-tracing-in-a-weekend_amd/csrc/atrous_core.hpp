// atrous_core.hpp — the arithmetic of the variance-guided a-trous wavelet filter (include/rt/rt_abi.h,
// rt_denoise_atrous), one definition for the device kernel (atrous_kernel.hip) and the host filter
// (atrous_host.cpp): the tap weight, the albedo clamp A', the initial state, the Vbar rule, the
// per-pixel level update over an accessor, and the output expressions. The luminance, the
// finite-value test and the feature term are denoise_core.hpp's. Compiled without contraction and
// without fast math, so both sides do the same f64 operations in the same order. Compiles without
// HIP: atrous_host.cpp is plain C++.
#pragma once

#include "denoise_core.hpp"

namespace rtk {

constexpr int kAtrousMaxLevels = 6;

// the state of one pixel: the colour and the variance of its luminance, one aligned 32-byte record
// (two 16-byte loads; Y is recomputed from it: a fifth double would break the alignment)
struct alignas(32) AtrousRec {
    double c0, c1, c2, v;
};

// h = (1/16, 1/4, 3/8, 1/4, 1/16) at d = -2..2
RT_DN_HD inline double atrous_h(int d)
{
    return d == 0 ? 0.375 : (d == 1 || d == -1) ? 0.25 : 0.0625;
}

// h(dx, dy) = h[dy + 2] * h[dx + 2]
RT_DN_HD inline double atrous_tap_weight(int dx, int dy)
{
    return atrous_h(dy) * atrous_h(dx);
}

// A' of one albedo channel: the divisor of the demodulated colour
RT_DN_HD inline double atrous_albedo(double a)
{
    if (!denoise_finite(a)) return 1.0;
    return a > 0.01 ? a : 0.01;
}

RT_DN_HD inline double atrous_luma(const AtrousRec& r)
{
    return denoise_luma(r.c0, r.c1, r.c2);
}

// state 0 of a pixel from its mean colour and standard error; a = its albedo, or null: not demodulated
RT_DN_HD inline AtrousRec atrous_initial(double m0, double m1, double m2, double se, const double* a)
{
    AtrousRec r;
    if (!a) {
        r.c0 = m0;
        r.c1 = m1;
        r.c2 = m2;
        r.v = se * se;
        return r;
    }
    const double a0 = atrous_albedo(a[0]), a1 = atrous_albedo(a[1]), a2 = atrous_albedo(a[2]);
    const double ya = denoise_luma(a0, a1, a2);
    r.c0 = m0 / a0;
    r.c1 = m1 / a1;
    r.c2 = m2 / a2;
    r.v = se * se / (ya * ya);
    return r;
}

// out(p) and stderr_out(p) from state L; a as above
RT_DN_HD inline void atrous_final(const AtrousRec& r, const double* a, double out[3], double& se_out)
{
    if (!a) {
        out[0] = r.c0;
        out[1] = r.c1;
        out[2] = r.c2;
        se_out = ::sqrt(r.v);
        return;
    }
    const double a0 = atrous_albedo(a[0]), a1 = atrous_albedo(a[1]), a2 = atrous_albedo(a[2]);
    const double ya = denoise_luma(a0, a1, a2);
    out[0] = r.c0 * a0;
    out[1] = r.c1 * a1;
    out[2] = r.c2 * a2;
    se_out = ::sqrt(r.v * (ya * ya));
}

// Vbar(p): the 3 x 3 binomial mean of V around (x, y) at distance 1, over the neighbours inside the
// image whose V is finite, divided by the weights taken, in raster order. acc.var(x, y) = V there.
template <typename Acc>
RT_DN_HD inline double atrous_vbar(const Acc& acc, int x, int y, int W, int H)
{
    double s = 0.0, ws = 0.0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const double v = acc.var(qx, qy);
            if (!denoise_finite(v)) continue;
            const double w = (dy == 0 ? 0.5 : 0.25) * (dx == 0 ? 0.5 : 0.25);
            s = s + w * v;
            ws = ws + w;
        }
    }
    return s / ws;
}

// State i + 1 of pixel (x, y) from state i, step s = 2^i. acc.load(x, y) = the record of state i at
// an inside pixel, acc.var(x, y) its V alone; guides with no frame: no feature term.
template <bool G, typename Acc>
RT_DN_HD inline AtrousRec atrous_level(const Acc& acc, const DenoiseGuides& guides, int x, int y, int W, int H, int s,
                                       double sigma_l)
{
    const AtrousRec c = acc.load(x, y);
    const double yc = atrous_luma(c);
    if (!denoise_finite(yc) || !denoise_finite(c.v)) return c;
    const double vbar = atrous_vbar(acc, x, y, W, H);
    const double dl = sigma_l * ::sqrt(vbar > 0.0 ? vbar : 0.0) + 1e-10;
    const size_t p = (size_t)y * (size_t)W + (size_t)x;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, sw = 0.0, sv = 0.0;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + s * dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + s * dx;
            if (qx < 0 || qx >= W) continue;
            AtrousRec q = c;
            double w = atrous_tap_weight(dx, dy);
            if (dx != 0 || dy != 0) {
                q = acc.load(qx, qy);
                double e = ::fabs(yc - atrous_luma(q)) / dl;
                if constexpr (G) e = e + denoise_phi(guides, p, (size_t)qy * (size_t)W + (size_t)qx);
                w = denoise_finite(e) && denoise_finite(q.v) ? w * ::exp(-e) : 0.0;
            }
            if (w == 0.0) continue;
            n0 = n0 + w * q.c0;
            n1 = n1 + w * q.c1;
            n2 = n2 + w * q.c2;
            sw = sw + w;
            sv = sv + w * w * q.v;
        }
    }
    AtrousRec r;
    r.c0 = n0 / sw;
    r.c1 = n1 / sw;
    r.c2 = n2 / sw;
    r.v = sv / (sw * sw);
    return r;
}

}  // namespace rtk
