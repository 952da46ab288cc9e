// pyramid.hpp — what the C ABI (abi_filters.cpp) needs of the multi-scale NL-means filter's two
// halves: the parameter check of pyramid_host.cpp (plain C++, links without HIP; with
// denoise_host.cpp, whose filter it runs per level) and the launcher of pyramid_kernel.hip, with the
// layout of the scratch the launcher works in. (The host entry's error hook: filter_guides.hpp.)
#pragma once

#include <stddef.h>

#include "rt/rt_abi.h"
#include "pyramid_core.hpp"

namespace rtk {

// rt_denoise_pyramid's and rt_denoise_pyramid_host's argument check: null when the call is valid
// (g may be null: no guides), else the text for rt_last_error (the code is RT_ERR_INVALID);
// G = the frames and 1 / sigma^2 of each guide given.
const char* pyramid_check(const rt_pyramid_params* p, const void* mean, const double* stderr_map,
                          const rt_denoise_guides* g, const void* out, DenoiseGuides& G);

// The f64 scratch frames of a device call, as offsets in doubles into one allocation. Level 0
// holds C_0 (only when the input is f32: the widened frame) and D_0; a level l >= 1 holds C_l,
// s_l, the guides given and D_l, which the Up pass turns into R_l in place; one correction frame K
// of level 1's size serves every level in turn. A call of one level needs none of it.
struct PyramidLayout {
    int levels = 0;
    int w[kPyramidMaxLevels] = {}, h[kPyramidMaxLevels] = {};
    size_t c[kPyramidMaxLevels] = {}, s[kPyramidMaxLevels] = {}, a[kPyramidMaxLevels] = {}, n[kPyramidMaxLevels] = {},
           z[kPyramidMaxLevels] = {}, d[kPyramidMaxLevels] = {};
    size_t k = 0;
    size_t doubles = 0;   // the whole scratch

    PyramidLayout(int width, int height, int levels_, bool f64, bool albedo, bool normal, bool depth) : levels(levels_)
    {
        w[0] = width, h[0] = height;
        for (int l = 1; l < levels; ++l) w[l] = pyramid_half(w[l - 1]), h[l] = pyramid_half(h[l - 1]);
        if (levels <= 1) return;
        size_t at = 0;
        auto take = [&at](size_t n_) { const size_t o = at; at += n_; return o; };
        for (int l = 0; l < levels; ++l) {
            const size_t hw = (size_t)w[l] * (size_t)h[l];
            if (l > 0 || !f64) c[l] = take(3 * hw);
            if (l > 0) {
                s[l] = take(hw);
                if (albedo) a[l] = take(3 * hw);
                if (normal) n[l] = take(3 * hw);
                if (depth) z[l] = take(hw);
            }
            d[l] = take(3 * hw);
        }
        k = take(3 * (size_t)w[1] * (size_t)h[1]);
        doubles = at;
    }
};

}  // namespace rtk

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace rtk {

// Where the filters of the levels above 0 run: a second stream and the two events that order it
// after Down (fork, recorded on the call's stream) and Up after it (join, recorded on side). A
// coarse level is too few workgroups to fill the device, so it runs beside level 0 instead of after
// it. A null side: every level on the call's stream, in order.
struct PyramidSide {
    hipStream_t side = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
};

// The filter of rt_abi.h over device buffers (f64: mean and out are double, else float): at one
// level launch_denoise on the caller's buffers; else widen (f32), Down, launch_denoise per level on
// the scratch's f64 frames, and Up. scratch: PyramidLayout(...).doubles doubles (null at one level).
// Everything the call enqueues anywhere is complete when what it enqueued on `stream` is.
hipError_t launch_pyramid(const void* mean, const double* se, void* out, bool f64, int width, int height, int radius,
                          int patch, double k, int levels, const DenoiseGuides& guides, double* scratch,
                          hipStream_t stream, const PyramidSide& side);

}  // namespace rtk
#endif
