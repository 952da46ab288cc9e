// cross.hpp — what the C ABI (abi_filters.cpp) needs of the cross-filtered NL-means' two halves:
// the parameter check of cross_host.cpp (plain C++, links without HIP and without the rest of the
// library) and the launcher of cross_kernel.hip. (The guide check and the host entry's error hook:
// filter_guides.hpp.)
#pragma once

#include "rt/rt_abi.h"
#include "denoise_core.hpp"

namespace rtk {

// rt_denoise_cross's and rt_denoise_cross_host's argument check: null when the call is valid, else
// the text for rt_last_error (the code is RT_ERR_INVALID).
const char* cross_check(const rt_cross_params* p, const void* mean_a, const void* mean_b, const double* stderr_map,
                        const void* out, const double* stderr_out);

}  // namespace rtk

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace rtk {

// LDS bytes of one workgroup of the filter kernel for (radius, patch)
int cross_lds_bytes(int radius, int patch);
// out, and se_out when given, = the filter of rt_abi.h over device buffers (f64: the means and out
// are double, else float). e: height x width f64 of scratch, needed iff se_out is given. Guides with
// no frame: the unguided instantiation.
hipError_t launch_cross(const void* mean_a, const void* mean_b, const double* se, void* out, double* se_out, double* e,
                        bool f64, int width, int height, int radius, int patch, double k, double scale,
                        const DenoiseGuides& guides, hipStream_t stream);

}  // namespace rtk
#endif
