// denoise.hpp — what the C ABI (abi.cpp) needs of the NL-means filter's two halves: the
// parameter check and the error hook of denoise_host.cpp (plain C++, links without HIP and without
// abi.cpp) and the launcher of denoise_kernel.hip.
#pragma once

#include "rt/rt_abi.h"
#include "denoise_core.hpp"

namespace rtk {

// rt_denoise's and rt_denoise_host's argument check: null when the call is valid, else the text
// for rt_last_error (the code is RT_ERR_INVALID).
const char* denoise_check(const rt_denoise_params* p, const void* mean, const double* stderr_map, const void* out);

// rt_denoise_guided's guides: null when they are valid (g may be null: no guides), else the text;
// G = the frames and 1 / sigma^2 of each guide given.
const char* denoise_guides_check(const rt_denoise_guides* g, DenoiseGuides& G);

// Where rt_denoise_host reports its error text. abi.cpp points it at rt_last_error's slot when
// the library loads; a program that links denoise_host.cpp alone leaves it null.
extern void (*denoise_error_sink)(const char* msg);

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
