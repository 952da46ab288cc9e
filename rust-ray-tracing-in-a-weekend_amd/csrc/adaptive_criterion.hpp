// adaptive_criterion.hpp — the tile-adaptive sampling criterion (include/rt/rt_abi.h,
// rt_render_adaptive), one definition for the device kernels (adaptive_kernel.hip) and the host
// restatement (rt_adaptive_tile_errors_host). Compiled without contraction and without fast
// math, so both sides do the same f64 operations in the same order.
#pragma once

#include <hip/hip_runtime.h>

namespace rtk {

// Rec. 709 luminance, left to right
__host__ __device__ inline double adaptive_luma(double r, double g, double b)
{
    return 0.2126 * r + 0.7152 * g + 0.0722 * b;
}

struct PixelNoise {
    double se;   // standard error of the pixel's luminance mean
    double e;    // se / sqrt(max(mean luminance, 1e-4)): the error after the output's sqrt gamma (x 2)
};

// From a pixel's RGB sums, its sum of squared sample luminances q and its sample count n >= 2.
__host__ __device__ inline PixelNoise adaptive_pixel_noise(double sr, double sg, double sb, double q, double n)
{
    const double ys = adaptive_luma(sr, sg, sb);
    const double m = ys / n;
    double var = (q - ys * ys / n) / (n - 1.0);
    var = var > 0.0 ? var : 0.0;
    PixelNoise o;
    o.se = __builtin_sqrt(var / n);
    o.e = o.se / __builtin_sqrt(m > 1e-4 ? m : 1e-4);
    return o;
}

}  // namespace rtk
