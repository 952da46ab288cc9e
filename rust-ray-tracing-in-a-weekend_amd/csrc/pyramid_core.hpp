// pyramid_core.hpp — the arithmetic rt_denoise_pyramid (include/rt/rt_abi.h) adds around the
// NL-means filter, one definition for the device kernels (pyramid_kernel.hip) and the host filter
// (pyramid_host.cpp): a level's size, the block mean and the standard error of a block mean (Down),
// and the four-tap correction (Up). Compiled without contraction and without fast math, so both
// sides do the same f64 operations in the same order. Compiles without HIP, as denoise_core.hpp.
#pragma once

#include "denoise_core.hpp"

namespace rtk {

constexpr int kPyramidMaxLevels = 5;

// the next level's extent along one axis
RT_DN_HD inline int pyramid_half(int n)
{
    return (n + 1) / 2;
}

// Channel ch of the block mean of coarse pixel (cx, cy): the raster-order sum, from 0.0, of a
// W x H frame of nch interleaved channels over the block's pixels inside the frame, divided by
// their number (1, 2 or 4).
RT_DN_HD inline double pyramid_block_mean(const double* f, int nch, int ch, int W, int H, int cx, int cy)
{
    const int x0 = 2 * cx, y0 = 2 * cy;
    const int nx = x0 + 1 < W ? 2 : 1, ny = y0 + 1 < H ? 2 : 1;
    double s = 0.0;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) s = s + f[((size_t)(y0 + j) * (size_t)W + (size_t)(x0 + i)) * (size_t)nch + (size_t)ch];
    return s / (double)(nx * ny);
}

// The standard error of the block mean of independent pixels: sqrt(sum se se) / n, the sum in
// raster order from 0.0.
RT_DN_HD inline double pyramid_block_se(const double* se, int W, int H, int cx, int cy)
{
    const int x0 = 2 * cx, y0 = 2 * cy;
    const int nx = x0 + 1 < W ? 2 : 1, ny = y0 + 1 < H ? 2 : 1;
    double t = 0.0;
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            const double s = se[(size_t)(y0 + j) * (size_t)W + (size_t)(x0 + i)];
            t = t + s * s;
        }
    return ::sqrt(t) / (double)(nx * ny);
}

// the second tap's coarse coordinate along one axis for fine coordinate x: the coarse neighbour on
// x's side of its block, clamped into [0, wc)
RT_DN_HD inline int pyramid_other(int x, int wc)
{
    const int c = x / 2;
    int o = (x & 1) ? c + 1 : c - 1;
    o = o < 0 ? 0 : o;
    return o > wc - 1 ? wc - 1 : o;
}

// u(p) for the fine pixel (x, y) from the correction frame K (wc x hc x 3): the four taps in the
// contract's order with weights 9/16, 3/16, 3/16, 1/16, a tap taken if its three channels are
// finite, the weighted sum divided by the sum of the weights taken; 0 if none is.
RT_DN_HD inline void pyramid_correction(const double* K, int wc, int hc, int x, int y, double u[3])
{
    const int cx = x / 2, cy = y / 2, ox = pyramid_other(x, wc), oy = pyramid_other(y, hc);
    const int tx[4] = {cx, ox, cx, ox}, ty[4] = {cy, cy, oy, oy};
    const double tw[4] = {9.0 / 16.0, 3.0 / 16.0, 3.0 / 16.0, 1.0 / 16.0};
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, sw = 0.0;
    for (int t = 0; t < 4; ++t) {
        const double* k = K + ((size_t)ty[t] * (size_t)wc + (size_t)tx[t]) * 3;
        if (!denoise_finite(k[0]) || !denoise_finite(k[1]) || !denoise_finite(k[2])) continue;
        n0 = n0 + tw[t] * k[0];
        n1 = n1 + tw[t] * k[1];
        n2 = n2 + tw[t] * k[2];
        sw = sw + tw[t];
    }
    const bool any = sw > 0.0;
    u[0] = any ? n0 / sw : 0.0;
    u[1] = any ? n1 / sw : 0.0;
    u[2] = any ? n2 / sw : 0.0;
}

}  // namespace rtk
