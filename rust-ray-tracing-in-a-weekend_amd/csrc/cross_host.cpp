// cross_host.cpp — rt_denoise_cross_host: the cross-filtered NL-means of include/rt/rt_abi.h on the
// host: nlm_host.hpp's filter with two halves (the device kernels' arithmetic). Plain C++: no
// HIP, and nothing from the rest of the library, so a test program can link this file alone.
#include <new>

#include "rt/rt_abi.h"
#include "cross.hpp"
#include "filter_guides.hpp"
#include "nlm_host.hpp"

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
    if (const char* bad = nlm_check_params(p->format, p->width, p->height, p->radius, p->patch, p->k)) return bad;
    if (!(p->variance_scale > 0.0) || !denoise_finite(p->variance_scale))
        return "variance_scale must be greater than 0 and finite";
    return nullptr;
}

namespace {

template <typename T>
void filter(const rt_cross_params& p, const void* mean_a, const void* mean_b, const double* se, const DenoiseGuides& G,
            void* out, double* se_out)
{
    const T* const M[2] = {(const T*)mean_a, (const T*)mean_b};
    nlm_filter<T, 2>(NlmWindow{p.width, p.height, p.radius, p.patch, p.k}, M, se, p.variance_scale, G, (T*)out, se_out);
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
        if (p->format == RT_OUT_F64) rtk::filter<double>(*p, mean_a, mean_b, stderr_map, G, out, stderr_out);
        else rtk::filter<float>(*p, mean_a, mean_b, stderr_map, G, out, stderr_out);
    } catch (const std::bad_alloc&) {
        return rtk::filter_fail(RT_ERR_OOM, "rt_denoise_cross_host: frame-sized work arrays");
    }
    return RT_OK;
}
