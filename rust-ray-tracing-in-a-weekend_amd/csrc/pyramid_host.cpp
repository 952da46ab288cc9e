// pyramid_host.cpp — rt_denoise_pyramid_host: the multi-scale NL-means filter of
// include/rt/rt_abi.h on the host, with pyramid_core.hpp's arithmetic (the device kernels') around
// rt_denoise_guided_host per level, and the argument check both entries share. Plain C++: no HIP,
// and of the rest of the library only denoise_host.cpp, so a test program can link the two alone.
#include <new>
#include <vector>

#include "rt/rt_abi.h"
#include "denoise.hpp"
#include "filter_guides.hpp"
#include "pyramid.hpp"
#include "pyramid_core.hpp"

namespace rtk {

const char* pyramid_check(const rt_pyramid_params* p, const void* mean, const double* stderr_map,
                          const rt_denoise_guides* g, const void* out, DenoiseGuides& G)
{
    G = DenoiseGuides{};
    if (!p) return "null argument";
    const rt_denoise_params d{p->width, p->height, p->format, p->on_device, p->radius, p->patch, p->k, p->stream};
    if (const char* bad = denoise_check(&d, mean, stderr_map, out)) return bad;
    if (p->levels < 1 || p->levels > kPyramidMaxLevels) return "levels out of range (1..5)";
    if (p->reserved0 != 0) return "reserved0 must be 0";
    return guides_check(g, G);
}

namespace {

// one level's f64 frames (a guide not given stays empty)
struct Level {
    int w = 0, h = 0;
    std::vector<double> c, s, a, n, z, d;
};

void block_means(const double* f, int nch, int W, int H, int wc, int hc, std::vector<double>& out)
{
    out.resize((size_t)wc * hc * nch);
    for (int cy = 0; cy < hc; ++cy)
        for (int cx = 0; cx < wc; ++cx)
            for (int ch = 0; ch < nch; ++ch)
                out[((size_t)cy * wc + cx) * nch + ch] = pyramid_block_mean(f, nch, ch, W, H, cx, cy);
}

// D = rt_denoise_guided's filter on a level's f64 frames
int filter_level(const rt_pyramid_params& p, const rt_denoise_guides* g, const Level& lv, const double* c,
                 const double* s, const double* a, const double* n, const double* z, double* d)
{
    const rt_denoise_params dp{lv.w, lv.h, RT_OUT_F64, 0, p.radius, p.patch, p.k, nullptr};
    rt_denoise_guides lg{};
    if (g) {
        lg = *g;
        lg.albedo = g->albedo ? a : nullptr;
        lg.normal = g->normal ? n : nullptr;
        lg.depth = g->depth ? z : nullptr;
    }
    return rt_denoise_guided_host(&dp, c, s, g ? &lg : nullptr, d);
}

template <typename T>
int filter(const rt_pyramid_params& p, const T* M, const double* se, const rt_denoise_guides* g, T* out)
{
    const int L = p.levels;
    const size_t hw = (size_t)p.width * (size_t)p.height;
    std::vector<Level> lv((size_t)L);
    lv[0].w = p.width, lv[0].h = p.height;
    lv[0].c.resize(3 * hw);
    for (size_t i = 0; i < 3 * hw; ++i) lv[0].c[i] = (double)M[i];
    // a level's frames: the caller's (widened) at level 0, the level's own above
    auto S = [&](int l) { return l ? lv[l].s.data() : se; };
    auto A = [&](int l) { return l ? lv[l].a.data() : g ? g->albedo : nullptr; };
    auto N = [&](int l) { return l ? lv[l].n.data() : g ? g->normal : nullptr; };
    auto Z = [&](int l) { return l ? lv[l].z.data() : g ? g->depth : nullptr; };
    for (int l = 0; l + 1 < L; ++l) {
        const int W = lv[l].w, H = lv[l].h, wc = pyramid_half(W), hc = pyramid_half(H);
        Level& up = lv[l + 1];
        up.w = wc, up.h = hc;
        block_means(lv[l].c.data(), 3, W, H, wc, hc, up.c);
        up.s.resize((size_t)wc * hc);
        for (int cy = 0; cy < hc; ++cy)
            for (int cx = 0; cx < wc; ++cx) up.s[(size_t)cy * wc + cx] = pyramid_block_se(S(l), W, H, cx, cy);
        if (g && g->albedo) block_means(A(l), 3, W, H, wc, hc, up.a);
        if (g && g->normal) block_means(N(l), 3, W, H, wc, hc, up.n);
        if (g && g->depth) block_means(Z(l), 1, W, H, wc, hc, up.z);
    }
    for (int l = 0; l < L; ++l) {
        lv[l].d.resize(3 * (size_t)lv[l].w * lv[l].h);
        const int rc = filter_level(p, g, lv[l], lv[l].c.data(), S(l), A(l), N(l), Z(l), lv[l].d.data());
        if (rc != RT_OK) return rc;
    }
    // Up: d becomes R in place, level by level
    std::vector<double> K;
    for (int l = L - 2; l >= 0; --l) {
        const int W = lv[l].w, H = lv[l].h, wc = lv[l + 1].w, hc = lv[l + 1].h;
        block_means(lv[l].d.data(), 3, W, H, wc, hc, K);
        for (size_t i = 0; i < K.size(); ++i) K[i] = lv[l + 1].d[i] - K[i];
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double u[3];
                pyramid_correction(K.data(), wc, hc, x, y, u);
                double* const r = lv[l].d.data() + ((size_t)y * W + x) * 3;
                for (int ch = 0; ch < 3; ++ch) r[ch] = r[ch] + u[ch];
            }
    }
    for (size_t i = 0; i < hw; ++i) {
        const bool keep = !denoise_finite(denoise_luma((double)M[3 * i], (double)M[3 * i + 1], (double)M[3 * i + 2])) ||
                          !denoise_finite(se[i]);
        for (int ch = 0; ch < 3; ++ch) out[3 * i + ch] = keep ? M[3 * i + ch] : (T)lv[0].d[3 * i + ch];
    }
    return RT_OK;
}

}  // namespace
}  // namespace rtk

extern "C" int rt_denoise_pyramid_host(const rt_pyramid_params* p, const void* mean, const double* stderr_map,
                                       const rt_denoise_guides* g, void* out)
{
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::pyramid_check(p, mean, stderr_map, g, out, G)) return rtk::filter_fail(RT_ERR_INVALID, bad);
    if (p->levels == 1) {   // the filter itself, on the caller's buffers
        const rt_denoise_params d{p->width, p->height, p->format, 0, p->radius, p->patch, p->k, nullptr};
        return rt_denoise_guided_host(&d, mean, stderr_map, g, out);
    }
    try {
        if (p->format == RT_OUT_F64) return rtk::filter<double>(*p, (const double*)mean, stderr_map, g, (double*)out);
        return rtk::filter<float>(*p, (const float*)mean, stderr_map, g, (float*)out);
    } catch (const std::bad_alloc&) {
        return rtk::filter_fail(RT_ERR_OOM, "rt_denoise_pyramid_host: frame-sized level arrays");
    }
}
