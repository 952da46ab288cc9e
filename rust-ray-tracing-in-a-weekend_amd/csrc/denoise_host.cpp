// denoise_host.cpp — rt_denoise_host and rt_denoise_guided_host: the variance-guided NL-means
// filter of include/rt/rt_abi.h, without and with feature guides, on the host: nlm_host.hpp's
// filter with one half (the device kernel's arithmetic). Plain C++: no HIP, and
// nothing from the rest of the library, so a test program can link this file alone.
#include <new>

#include "rt/rt_abi.h"
#include "denoise.hpp"
#include "filter_guides.hpp"
#include "nlm_host.hpp"

namespace rtk {

const char* denoise_check(const rt_denoise_params* p, const void* mean, const double* stderr_map, const void* out)
{
    if (!p || !mean || !stderr_map || !out) return "null argument";
    if (out == mean) return "rt_denoise does not filter in place: out == mean";
    return nlm_check_params(p->format, p->width, p->height, p->radius, p->patch, p->k);
}

namespace {

template <typename T>
void filter(const rt_denoise_params& p, const void* mean, const double* se, const DenoiseGuides& G, void* out)
{
    const T* const M[1] = {(const T*)mean};
    nlm_filter<T, 1>(NlmWindow{p.width, p.height, p.radius, p.patch, p.k}, M, se, 1.0, G, (T*)out, nullptr);
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
        if (p->format == RT_OUT_F64) rtk::filter<double>(*p, mean, stderr_map, G, out);
        else rtk::filter<float>(*p, mean, stderr_map, G, out);
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
