// cross_host.cpp — rt_denoise_cross_host: the cross-filtered NL-means of include/rt/rt_abi.h on the
// host, with denoise_core.hpp's and cross_core.hpp's arithmetic (the device kernels'). Plain C++: no
// HIP, and nothing from the rest of the library, so a test program can link this file alone.
#include <cmath>
#include <new>
#include <vector>

#include "rt/rt_abi.h"
#include "cross.hpp"
#include "cross_core.hpp"
#include "filter_guides.hpp"

namespace rtk {

const char* cross_check(const rt_cross_params* p, const void* mean_a, const void* mean_b, const double* stderr_map,
                        const void* out, const double* stderr_out)
{
    if (!p || !mean_a || !mean_b || !stderr_map || !out) return "null argument";
    if (out == mean_a || out == mean_b || out == (const void*)stderr_map)
        return "rt_denoise_cross does not filter in place: out is one of the inputs";
    if (stderr_out && (stderr_out == stderr_map || (const void*)stderr_out == mean_a || (const void*)stderr_out == mean_b ||
                       (const void*)stderr_out == out))
        return "stderr_out is one of the other frames";
    if (p->format != RT_OUT_F32 && p->format != RT_OUT_F64) return "bad format";
    if (p->width < 1 || p->height < 1 || (long long)p->width * p->height > 0xffffffffLL) return "bad frame size";
    if (p->radius < 1 || p->radius > kDenoiseMaxRadius) return "radius out of range (1..10)";
    if (p->patch < 0 || p->patch > kDenoiseMaxPatch) return "patch out of range (0..3)";
    if (!(p->k > 0.0) || !denoise_finite(p->k)) return "k must be greater than 0 and finite";
    if (!(p->variance_scale > 0.0) || !denoise_finite(p->variance_scale))
        return "variance_scale must be greater than 0 and finite";
    return nullptr;
}

namespace {

template <typename T>
void filter(const rt_cross_params& p, const T* MA, const T* MB, const double* se, const DenoiseGuides& G, T* out,
            double* se_out)
{
    const bool guided = G.any();
    const int W = p.width, H = p.height, r = p.radius, f = p.patch;
    const size_t hw = (size_t)W * (size_t)H;
    const double k2 = p.k * p.k;
    std::vector<double> YA(hw), YB(hw), V(hw), delta_a(hw), delta_b(hw);
    std::vector<double> num_a(3 * hw, 0.0), num_b(3 * hw, 0.0), den_a(hw, 0.0), den_b(hw, 0.0);
    for (size_t i = 0; i < hw; ++i) {
        const CrossCell c = cross_cell((double)MA[3 * i], (double)MA[3 * i + 1], (double)MA[3 * i + 2], (double)MB[3 * i],
                                       (double)MB[3 * i + 1], (double)MB[3 * i + 2], se[i], p.variance_scale);
        YA[i] = c.ya;
        YB[i] = c.yb;
        V[i] = c.v;
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
                        delta_a[a] = denoise_delta(YA[a], V[a], YA[b], V[b], k2);
                        delta_b[a] = denoise_delta(YB[a], V[a], YB[b], V[b], k2);
                    }
                }
            }
            for (int y = y0; y < y1; ++y) {
                const int sy0 = y - f > y0 ? y - f : y0, sy1 = y + f < y1 - 1 ? y + f : y1 - 1;
                for (int x = x0; x < x1; ++x) {
                    const size_t a = (size_t)y * W + x, b = (size_t)(y + dy) * W + (x + dx);
                    double wa = 1.0, wb = 1.0;
                    if (!centre) {
                        const int sx0 = x - f > x0 ? x - f : x0, sx1 = x + f < x1 - 1 ? x + f : x1 - 1;
                        double sa = 0.0, sb = 0.0;
                        for (int sy = sy0; sy <= sy1; ++sy) {
                            for (int sx = sx0; sx <= sx1; ++sx) {
                                sa = sa + delta_a[(size_t)sy * W + sx];
                                sb = sb + delta_b[(size_t)sy * W + sx];
                            }
                        }
                        const double cnt = (double)((sx1 - sx0 + 1) * (sy1 - sy0 + 1));
                        const double Da = sa / cnt, Db = sb / cnt;
                        if (guided) {
                            const double phi = denoise_phi(G, a, b);
                            wa = denoise_weight_guided(Da, phi);
                            wb = denoise_weight_guided(Db, phi);
                        } else {
                            wa = denoise_weight(Da);
                            wb = denoise_weight(Db);
                        }
                    }
                    // cross application: half B's weights filter half A and the reverse
                    if (wb != 0.0) {
                        num_a[3 * a + 0] = num_a[3 * a + 0] + wb * (double)MA[3 * b + 0];
                        num_a[3 * a + 1] = num_a[3 * a + 1] + wb * (double)MA[3 * b + 1];
                        num_a[3 * a + 2] = num_a[3 * a + 2] + wb * (double)MA[3 * b + 2];
                        den_a[a] = den_a[a] + wb;
                    }
                    if (wa != 0.0) {
                        num_b[3 * a + 0] = num_b[3 * a + 0] + wa * (double)MB[3 * b + 0];
                        num_b[3 * a + 1] = num_b[3 * a + 1] + wa * (double)MB[3 * b + 1];
                        num_b[3 * a + 2] = num_b[3 * a + 2] + wa * (double)MB[3 * b + 2];
                        den_b[a] = den_b[a] + wa;
                    }
                }
            }
        }
    }
    std::vector<double> e(se_out ? hw : 0);
    for (size_t i = 0; i < hw; ++i) {
        const bool keep = cross_bad(YA[i]);
        double fa[3], fb[3];
        for (int c = 0; c < 3; ++c) {
            fa[c] = keep ? (double)MA[3 * i + c] : num_a[3 * i + c] / den_a[i];
            fb[c] = keep ? (double)MB[3 * i + c] : num_b[3 * i + c] / den_b[i];
            out[3 * i + c] = (T)(0.5 * (fa[c] + fb[c]));
        }
        if (se_out) e[i] = cross_half_diff(fa, fb);
    }
    if (se_out) {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) se_out[(size_t)y * W + x] = cross_stderr(e.data(), x, y, W, H);
    }
}

}  // namespace
}  // namespace rtk

extern "C" int rt_denoise_cross_host(const rt_cross_params* p, const void* mean_a, const void* mean_b,
                                     const double* stderr_map, const rt_denoise_guides* g, void* out, double* stderr_out)
{
    if (const char* bad = rtk::cross_check(p, mean_a, mean_b, stderr_map, out, stderr_out))
        return rtk::filter_fail(RT_ERR_INVALID, bad);
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::guides_check(g, G)) return rtk::filter_fail(RT_ERR_INVALID, bad);
    try {
        if (p->format == RT_OUT_F64)
            rtk::filter<double>(*p, (const double*)mean_a, (const double*)mean_b, stderr_map, G, (double*)out, stderr_out);
        else
            rtk::filter<float>(*p, (const float*)mean_a, (const float*)mean_b, stderr_map, G, (float*)out, stderr_out);
    } catch (const std::bad_alloc&) {
        return rtk::filter_fail(RT_ERR_OOM, "rt_denoise_cross_host: frame-sized work arrays");
    }
    return RT_OK;
}
