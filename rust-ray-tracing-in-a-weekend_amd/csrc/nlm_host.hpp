// nlm_host.hpp — the NL-means filter on the host, once: the offset loop over N frames that share one
// standard-error map, with denoise_core.hpp's and cross_core.hpp's arithmetic (the device kernels',
// denoise_kernel.hip and cross_kernel.hip). N = 1 is rt_denoise_host's and rt_denoise_guided_host's
// filter (denoise_host.cpp), N = 2 rt_denoise_cross_host's (cross_host.cpp). Plain C++ and a header:
// no HIP, and each of those two files still links alone into a test program.
#pragma once

#include <vector>

#include "rt/rt_abi.h"
#include "cross_core.hpp"
#include "denoise_core.hpp"

namespace rtk {

// What the argument checks of the NL-means filters share (denoise_check, cross_check): null when
// format, frame size, radius, patch and k are valid, else the text for rt_last_error.
inline const char* nlm_check_params(int format, int width, int height, int radius, int patch, double k)
{
    if (format != RT_OUT_F32 && format != RT_OUT_F64) return "bad format";
    if (width < 1 || height < 1 || (long long)width * height > 0xffffffffLL) return "bad frame size";
    if (radius < 1 || radius > kDenoiseMaxRadius) return "radius out of range (1..10)";
    if (patch < 0 || patch > kDenoiseMaxPatch) return "patch out of range (0..3)";
    if (!(k > 0.0) || !denoise_finite(k)) return "k must be greater than 0 and finite";
    return nullptr;
}

struct NlmWindow {
    int width, height, radius, patch;
    double k;
};

// out = the filter of N halves M[0..N) under the window p; half n's sums take the weights of half
// N - 1 - n (with one half, its own). One half: Y and V = se^2 as they are, and M kept where either
// is not finite. Two: cross_cell's Y_A, Y_B and V = scale se^2, the average of the two filtered
// halves, and se_out (when given) from their difference. Throws std::bad_alloc.
template <typename T, int N>
void nlm_filter(const NlmWindow& p, const T* const (&M)[N], const double* se, double scale, const DenoiseGuides& G, T* out,
                double* se_out)
{
    static_assert(N == 1 || N == 2, "one frame or two halves");
    const bool guided = G.any();
    const int W = p.width, H = p.height, r = p.radius, f = p.patch;
    const size_t hw = (size_t)W * (size_t)H;
    const double k2 = p.k * p.k;
    std::vector<double> Y[N], V(hw), delta[N], num[N], den[N];
    for (int n = 0; n < N; ++n) {
        Y[n].resize(hw);
        delta[n].resize(hw);
        num[n].assign(3 * hw, 0.0);
        den[n].assign(hw, 0.0);
    }
    for (size_t i = 0; i < hw; ++i) {
        if constexpr (N == 1) {
            Y[0][i] = denoise_luma((double)M[0][3 * i], (double)M[0][3 * i + 1], (double)M[0][3 * i + 2]);
            V[i] = se[i] * se[i];
        } else {
            const CrossCell c = cross_cell((double)M[0][3 * i], (double)M[0][3 * i + 1], (double)M[0][3 * i + 2],
                                           (double)M[1][3 * i], (double)M[1][3 * i + 1], (double)M[1][3 * i + 2], se[i],
                                           scale);
            Y[0][i] = c.ya;
            Y[1][i] = c.yb;
            V[i] = c.v;
        }
    }
    // offsets in raster order, so every pixel accumulates its terms in that order
    for (int dy = -r; dy <= r; ++dy) {
        for (int dx = -r; dx <= r; ++dx) {
            // the pairs (a, a + o) with both ends inside the image
            const int x0 = dx < 0 ? -dx : 0, x1 = dx > 0 ? W - dx : W;
            const int y0 = dy < 0 ? -dy : 0, y1 = dy > 0 ? H - dy : H;
            if (x0 >= x1 || y0 >= y1) continue;
            const bool centre = dx == 0 && dy == 0;
            if (!centre) {
                for (int y = y0; y < y1; ++y) {
                    for (int x = x0; x < x1; ++x) {
                        const size_t a = (size_t)y * W + x, b = (size_t)(y + dy) * W + (x + dx);
                        for (int n = 0; n < N; ++n) delta[n][a] = denoise_delta(Y[n][a], V[a], Y[n][b], V[b], k2);
                    }
                }
            }
            for (int y = y0; y < y1; ++y) {
                const int sy0 = y - f > y0 ? y - f : y0, sy1 = y + f < y1 - 1 ? y + f : y1 - 1;
                for (int x = x0; x < x1; ++x) {
                    const size_t a = (size_t)y * W + x, b = (size_t)(y + dy) * W + (x + dx);
                    double w[N];
                    for (int n = 0; n < N; ++n) w[n] = 1.0;
                    if (!centre) {
                        const int sx0 = x - f > x0 ? x - f : x0, sx1 = x + f < x1 - 1 ? x + f : x1 - 1;
                        double s[N] = {};
                        for (int sy = sy0; sy <= sy1; ++sy)
                            for (int sx = sx0; sx <= sx1; ++sx)
                                for (int n = 0; n < N; ++n) s[n] = s[n] + delta[n][(size_t)sy * W + sx];
                        const double cnt = (double)((sx1 - sx0 + 1) * (sy1 - sy0 + 1));
                        const double phi = guided ? denoise_phi(G, a, b) : 0.0;   // once for all halves
                        for (int n = 0; n < N; ++n)
                            w[n] = guided ? denoise_weight_guided(s[n] / cnt, phi) : denoise_weight(s[n] / cnt);
                    }
                    // cross application: half B's weights filter half A and the reverse
                    for (int n = 0; n < N; ++n) {
                        const double wn = w[N - 1 - n];
                        if (wn == 0.0) continue;
                        num[n][3 * a + 0] = num[n][3 * a + 0] + wn * (double)M[n][3 * b + 0];
                        num[n][3 * a + 1] = num[n][3 * a + 1] + wn * (double)M[n][3 * b + 1];
                        num[n][3 * a + 2] = num[n][3 * a + 2] + wn * (double)M[n][3 * b + 2];
                        den[n][a] = den[n][a] + wn;
                    }
                }
            }
        }
    }
    if constexpr (N == 1) {
        for (size_t i = 0; i < hw; ++i) {
            const bool keep = !denoise_finite(Y[0][i]) || !denoise_finite(V[i]);
            for (int c = 0; c < 3; ++c) out[3 * i + c] = keep ? M[0][3 * i + c] : (T)(num[0][3 * i + c] / den[0][i]);
        }
    } else {
        std::vector<double> e(se_out ? hw : 0);
        for (size_t i = 0; i < hw; ++i) {
            const bool keep = cross_bad(Y[0][i]);
            double fa[3], fb[3];
            for (int c = 0; c < 3; ++c) {
                fa[c] = keep ? (double)M[0][3 * i + c] : num[0][3 * i + c] / den[0][i];
                fb[c] = keep ? (double)M[1][3 * i + c] : num[1][3 * i + c] / den[1][i];
                out[3 * i + c] = (T)(0.5 * (fa[c] + fb[c]));
            }
            if (se_out) e[i] = cross_half_diff(fa, fb);
        }
        if (se_out) {
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) se_out[(size_t)y * W + x] = cross_stderr(e.data(), x, y, W, H);
        }
    }
}

}  // namespace rtk
