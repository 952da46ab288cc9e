// features_kernel.hpp — launch interface of rt_render_features' kernels (features_kernel.hip; the
// per-variant trace_features instantiations live in features_v_*.hip over features_device.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "trace_kernel.hpp"

namespace rtk {

// doubles of one (pixel, chunk) partial: albedo rgb, normal xyz, depth
constexpr int kFeatureChannels = 7;

// The first-hit pass over chunks [0, Ph.n_chunks) of samples starting at Ph.sample_begin (the
// chunk schedule's geometry: KParams as rt_render fills it for a whole frame). partial =
// [chunk][pixel][7] sums. o: the plan's features, slab32, lds_stack (f64 only: o.f32 and o.count
// must be 0, else hipErrorNotSupported).
hipError_t launch_features(const SceneDev& S, const KParams& Ph, const KParams* P, double* partial,
                           const LaunchOpts& o, hipStream_t stream);

// Per pixel: acc (n_px x 7; first: taken as 0.0) + the partials in chunk order; last: the three
// frames (any may be null) = the sums * scale, else the sums go back to acc for the next batch.
hipError_t launch_reduce_features(const double* partial, double* acc, double* albedo, double* normal, double* depth,
                                  long long n_px, int n_chunks, bool first, bool last, double scale,
                                  hipStream_t stream);

}  // namespace rtk
