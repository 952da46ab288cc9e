// denoise.hpp — what the C ABI (abi_filters.cpp) needs of the NL-means filter's two halves: the
// parameter check of denoise_host.cpp (plain C++, links without HIP and without the rest of the
// library) and the launcher of denoise_kernel.hip. (The guide check and the host entries' error
// hook, shared with the a-trous filter: filter_guides.hpp.)
#pragma once

#include "rt/rt_abi.h"
#include "denoise_core.hpp"

namespace rtk {

// rt_denoise's and rt_denoise_host's argument check: null when the call is valid, else the text
// for rt_last_error (the code is RT_ERR_INVALID).
const char* denoise_check(const rt_denoise_params* p, const void* mean, const double* stderr_map, const void* out);

}  // namespace rtk

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace rtk {

// LDS bytes of one workgroup of the kernel for (radius, patch)
int denoise_lds_bytes(int radius, int patch);
// out = the filter of rt_abi.h over device buffers (f64: mean and out are double, else float);
// guides with no frame: the unguided instantiation (rt_denoise's kernel)
hipError_t launch_denoise(const void* mean, const double* se, void* out, bool f64, int width, int height, int radius,
                          int patch, double k, const DenoiseGuides& guides, hipStream_t stream);

}  // namespace rtk
#endif
