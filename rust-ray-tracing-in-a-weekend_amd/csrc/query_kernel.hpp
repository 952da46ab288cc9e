// query_kernel.hpp — launch interface of rt_trace_rays' kernels (query_kernel.hip; the per-variant
// trace_query instantiations live in query_v_*.hip over query_device.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "rt/rt_abi.h"
#include "trace_kernel.hpp"

namespace rtk {

// One launch's rays and outputs (device pointers; rays and hits 16-byte aligned), passed by value.
struct QueryArgs {
    const rt_ray* rays;
    rt_hit* hits;            // CLOSEST: may be null
    double* albedo;          // CLOSEST: n x 3, may be null
    uint8_t* occluded;       // ANY
    long long n;
    uint64_t seed;           // the medium's keyed draw: (seed, ray.key_pixel, ray.key_sample, bounce)
    uint32_t bounce;
    int32_t has_moving;      // the scene holds a moving sphere: ray times outside [time_lo, time_hi] are flagged
    double time_lo, time_hi;
    double origin_bound;     // rays with an |o component| beyond it are flagged (+inf: none)
};

// mode: RT_QUERY_CLOSEST / RT_QUERY_ANY. o: the plan's features, slab32, lds_stack (f64 only: o.f32
// and o.count must be 0, else hipErrorNotSupported). Q.n = 0 launches nothing.
hipError_t launch_query(const SceneDev& S, const QueryArgs& Q, int mode, const LaunchOpts& o, hipStream_t stream);

}  // namespace rtk
