// atrous_host.cpp — rt_denoise_atrous_host: the variance-guided a-trous wavelet filter of
// include/rt/rt_abi.h on the host, with atrous_core.hpp's arithmetic (the device kernel's), and the
// argument check both entries share. Plain C++: no HIP, and nothing from the rest of the library,
// so a test program can link this file alone.
#include <new>
#include <vector>

#include "rt/rt_abi.h"
#include "atrous.hpp"
#include "atrous_core.hpp"
#include "filter_guides.hpp"

namespace rtk {

const char* atrous_check(const rt_atrous_params* p, const void* mean, const double* stderr_map,
                         const rt_denoise_guides* g, const void* out, const double* stderr_out, DenoiseGuides& G)
{
    G = DenoiseGuides{};
    if (!p || !mean || !stderr_map || !out) return "null argument";
    if (out == mean) return "rt_denoise_atrous does not filter in place: out == mean";
    if (stderr_out == stderr_map) return "rt_denoise_atrous does not filter in place: stderr_out == stderr_map";
    if (p->format != RT_OUT_F32 && p->format != RT_OUT_F64) return "bad format";
    if (p->width < 1 || p->height < 1 || (long long)p->width * p->height > 0xffffffffLL) return "bad frame size";
    if (p->levels < 1 || p->levels > kAtrousMaxLevels) return "levels out of range (1..6)";
    if (!(p->sigma_l > 0.0) || !denoise_finite(p->sigma_l)) return "sigma_l must be greater than 0 and finite";
    if (p->demodulate != 0 && p->demodulate != 1) return "demodulate must be 0 or 1";
    if (p->demodulate && (!g || !g->albedo)) return "demodulate needs an albedo guide";
    return guides_check(g, G);
}

namespace {

// a level's view of a frame of state records
struct StateAccess {
    const AtrousRec* s;
    int W;
    AtrousRec load(int x, int y) const { return s[(size_t)y * (size_t)W + (size_t)x]; }
    double var(int x, int y) const { return s[(size_t)y * (size_t)W + (size_t)x].v; }
};

template <typename T>
void filter(const rt_atrous_params& p, const T* M, const double* se, const DenoiseGuides& G, T* out, double* se_out)
{
    const bool guided = G.any();
    const int W = p.width, H = p.height;
    const size_t hw = (size_t)W * (size_t)H;
    const double* const albedo = p.demodulate ? G.albedo : nullptr;
    std::vector<AtrousRec> a(hw), b(hw);
    for (size_t i = 0; i < hw; ++i)
        a[i] = atrous_initial((double)M[3 * i], (double)M[3 * i + 1], (double)M[3 * i + 2], se[i],
                              albedo ? albedo + 3 * i : nullptr);
    for (int level = 0; level < p.levels; ++level) {
        const StateAccess acc{a.data(), W};
        const int s = 1 << level;
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                b[(size_t)y * W + x] = guided ? atrous_level<true>(acc, G, x, y, W, H, s, p.sigma_l)
                                              : atrous_level<false>(acc, G, x, y, W, H, s, p.sigma_l);
        a.swap(b);
    }
    for (size_t i = 0; i < hw; ++i) {
        double c[3], s;
        atrous_final(a[i], albedo ? albedo + 3 * i : nullptr, c, s);
        const bool keep = !denoise_finite(denoise_luma((double)M[3 * i], (double)M[3 * i + 1], (double)M[3 * i + 2])) ||
                          !denoise_finite(se[i]);
        for (int k = 0; k < 3; ++k) out[3 * i + k] = keep ? M[3 * i + k] : (T)c[k];
        if (se_out) se_out[i] = s;
    }
}

}  // namespace
}  // namespace rtk

extern "C" int rt_denoise_atrous_host(const rt_atrous_params* p, const void* mean, const double* stderr_map,
                                      const rt_denoise_guides* g, void* out, double* stderr_out)
{
    rtk::DenoiseGuides G;
    if (const char* bad = rtk::atrous_check(p, mean, stderr_map, g, out, stderr_out, G))
        return rtk::filter_fail(RT_ERR_INVALID, bad);
    try {
        if (p->format == RT_OUT_F64) rtk::filter<double>(*p, (const double*)mean, stderr_map, G, (double*)out, stderr_out);
        else rtk::filter<float>(*p, (const float*)mean, stderr_map, G, (float*)out, stderr_out);
    } catch (const std::bad_alloc&) {
        return rtk::filter_fail(RT_ERR_OOM, "rt_denoise_atrous_host: frame-sized state arrays");
    }
    return RT_OK;
}
