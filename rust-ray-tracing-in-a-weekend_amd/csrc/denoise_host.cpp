// denoise_host.cpp — rt_denoise_host and rt_denoise_guided_host: the variance-guided NL-means
// filter of include/rt/rt_abi.h, without and with feature guides, on the host, with
// denoise_core.hpp's arithmetic (the device kernel's). Plain C++: no HIP, and
// nothing from the rest of the library, so a test program can link this file alone.
#include <cmath>
#include <new>
#include <vector>

#include "rt/rt_abi.h"
#include "denoise.hpp"
#include "denoise_core.hpp"
#include "filter_guides.hpp"

namespace rtk {

const char* denoise_check(const rt_denoise_params* p, const void* mean, const double* stderr_map, const void* out)
{
    if (!p || !mean || !stderr_map || !out) return "null argument";
    if (out == mean) return "rt_denoise does not filter in place: out == mean";
    if (p->format != RT_OUT_F32 && p->format != RT_OUT_F64) return "bad format";
    if (p->width < 1 || p->height < 1 || (long long)p->width * p->height > 0xffffffffLL) return "bad frame size";
    if (p->radius < 1 || p->radius > kDenoiseMaxRadius) return "radius out of range (1..10)";
    if (p->patch < 0 || p->patch > kDenoiseMaxPatch) return "patch out of range (0..3)";
    if (!(p->k > 0.0) || !denoise_finite(p->k)) return "k must be greater than 0 and finite";
    return nullptr;
}

namespace {

template <typename T>
void filter(const rt_denoise_params& p, const T* M, const double* se, const DenoiseGuides& G, T* out)
{
    const bool guided = G.any();
    const int W = p.width, H = p.height, r = p.radius, f = p.patch;
    const size_t hw = (size_t)W * (size_t)H;
    const double k2 = p.k * p.k;
    std::vector<double> Y(hw), V(hw), delta(hw), num(3 * hw, 0.0), den(hw, 0.0);
    for (size_t i = 0; i < hw; ++i) {
        Y[i] = denoise_luma((double)M[3 * i], (double)M[3 * i + 1], (double)M[3 * i + 2]);
        V[i] = se[i] * se[i];
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
                        delta[a] = denoise_delta(Y[a], V[a], Y[b], V[b], k2);
                    }
                }
            }
            for (int y = y0; y < y1; ++y) {
                const int sy0 = y - f > y0 ? y - f : y0, sy1 = y + f < y1 - 1 ? y + f : y1 - 1;
                for (int x = x0; x < x1; ++x) {
                    const size_t a = (size_t)y * W + x, b = (size_t)(y + dy) * W + (x + dx);
                    double w = 1.0;
                    if (!centre) {
                        const int sx0 = x - f > x0 ? x - f : x0, sx1 = x + f < x1 - 1 ? x + f : x1 - 1;
                        double s = 0.0;
                        for (int sy = sy0; sy <= sy1; ++sy)
                            for (int sx = sx0; sx <= sx1; ++sx) s = s + delta[(size_t)sy * W + sx];
                        const double D = s / (double)((sx1 - sx0 + 1) * (sy1 - sy0 + 1));
                        w = guided ? denoise_weight_guided(D, denoise_phi(G, a, b)) : denoise_weight(D);
                    }
                    if (w == 0.0) continue;
                    num[3 * a + 0] = num[3 * a + 0] + w * (double)M[3 * b + 0];
                    num[3 * a + 1] = num[3 * a + 1] + w * (double)M[3 * b + 1];
                    num[3 * a + 2] = num[3 * a + 2] + w * (double)M[3 * b + 2];
                    den[a] = den[a] + w;
                }
            }
        }
    }
    for (size_t i = 0; i < hw; ++i) {
        const bool keep = !denoise_finite(Y[i]) || !denoise_finite(V[i]);
        for (int c = 0; c < 3; ++c) out[3 * i + c] = keep ? M[3 * i + c] : (T)(num[3 * i + c] / den[i]);
    }
}

}  // namespace
}  // namespace rtk

extern "C" int rt_denoise_guided_host(const rt_denoise_params* p, const void* mean, const double* stderr_map,
                                      const rt_denoise_guides* g, void* out)
{
    if (const char* bad = rtk::denoise_check(p, mean, stderr_map, out)) return rtk::filter_fail(RT_ERR_INVALID, bad);
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::guides_check(g, G)) return rtk::filter_fail(RT_ERR_INVALID, bad);
    try {
        if (p->format == RT_OUT_F64) rtk::filter<double>(*p, (const double*)mean, stderr_map, G, (double*)out);
        else rtk::filter<float>(*p, (const float*)mean, stderr_map, G, (float*)out);
    } catch (const std::bad_alloc&) {
        return rtk::filter_fail(RT_ERR_OOM, "rt_denoise_host: frame-sized work arrays");
    }
    return RT_OK;
}

// the guided filter with no guides
extern "C" int rt_denoise_host(const rt_denoise_params* p, const void* mean, const double* stderr_map, void* out)
{
    return rt_denoise_guided_host(p, mean, stderr_map, nullptr, out);
}
