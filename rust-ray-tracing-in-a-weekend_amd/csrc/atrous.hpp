// atrous.hpp — what the C ABI (abi_filters.cpp) needs of the a-trous filter's two halves: the
// parameter check of atrous_host.cpp (plain C++, links without HIP, without denoise_host.cpp and
// without the rest of the library) and the launcher of atrous_kernel.hip. (The host entry's error
// hook: filter_guides.hpp.)
#pragma once

#include "rt/rt_abi.h"
#include "atrous_core.hpp"

namespace rtk {

// rt_denoise_atrous's and rt_denoise_atrous_host's argument check: null when the call is valid
// (g may be null: no guides), else the text for rt_last_error (the code is RT_ERR_INVALID);
// G = the frames and 1 / sigma^2 of each guide given.
const char* atrous_check(const rt_atrous_params* p, const void* mean, const double* stderr_map,
                         const rt_denoise_guides* g, const void* out, const double* stderr_out, DenoiseGuides& G);

// state buffers a call of `levels` levels needs: 0, 1 or 2 (frame-sized arrays of AtrousRec)
inline int atrous_state_buffers(int levels) { return levels <= 1 ? 0 : levels == 2 ? 1 : 2; }

}  // namespace rtk

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace rtk {

// The filter of rt_abi.h over device buffers, one launch per level (f64: mean and out are double,
// else float). scratch: atrous_state_buffers(levels) consecutive arrays of width x height
// AtrousRec, 32-byte aligned; albedo: the demodulation's frame or null; stderr_out may be null.
hipError_t launch_atrous(const void* mean, const double* se, void* out, double* stderr_out, bool f64, int width,
                         int height, int levels, double sigma_l, const double* albedo, const DenoiseGuides& guides,
                         AtrousRec* scratch, hipStream_t stream);

}  // namespace rtk
#endif
