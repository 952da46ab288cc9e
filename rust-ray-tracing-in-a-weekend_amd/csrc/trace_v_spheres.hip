// trace_v_spheres.hip — instantiates the megakernel (trace_device.hpp) for one feature set
// (FEAT_SET_SPHERES, count_work false); each variant is its own translation unit so the build
// compiles them in parallel.
#include "trace_launch.hpp"

namespace rtk {
template hipError_t launch_variant<FEAT_SET_SPHERES, false>(const Launch&, const LaunchOpts&, hipStream_t);
}  // namespace rtk
