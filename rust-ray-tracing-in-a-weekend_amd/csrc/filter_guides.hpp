// filter_guides.hpp — what the two post-filters' host halves share: the check of a call's feature
// guides and the hook their host entries report errors through. Header-only and plain C++ (no HIP,
// included by no kernel), so denoise_host.cpp and atrous_host.cpp each still link alone.
#pragma once

#include "rt/rt_abi.h"
#include "denoise_core.hpp"

#pragma GCC visibility push(hidden)   // (private to the library: nothing here is exported from it)

namespace rtk {

// The guides of rt_denoise_guided and rt_denoise_atrous: null when they are valid (g may be null:
// no guides), else the text for rt_last_error (the code is RT_ERR_INVALID); G = the frames and
// 1 / sigma^2 of each guide given.
inline const char* guides_check(const rt_denoise_guides* g, DenoiseGuides& G)
{
    G = DenoiseGuides{};
    if (!g) return nullptr;
    auto bad = [](double s) { return !(s > 0.0) || !denoise_finite(s); };
    if ((g->albedo && bad(g->sigma_albedo)) || (g->normal && bad(g->sigma_normal)) || (g->depth && bad(g->sigma_depth)))
        return "the sigma of every guide given must be greater than 0 and finite";
    G.albedo = g->albedo;
    G.normal = g->normal;
    G.depth = g->depth;
    if (g->albedo) G.ia = 1.0 / (g->sigma_albedo * g->sigma_albedo);
    if (g->normal) G.in = 1.0 / (g->sigma_normal * g->sigma_normal);
    if (g->depth) G.iz = 1.0 / (g->sigma_depth * g->sigma_depth);
    return nullptr;
}

// Where rt_denoise_host, rt_denoise_guided_host and rt_denoise_atrous_host report their error
// text. The library points it at rt_last_error's slot when it loads (abi_filters.cpp); a program
// that links one of the host files alone leaves it null.
inline void (*filter_error_sink)(const char* msg) = nullptr;

inline int filter_fail(int code, const char* msg)
{
    if (filter_error_sink) filter_error_sink(msg);
    return code;
}

}  // namespace rtk

#pragma GCC visibility pop
