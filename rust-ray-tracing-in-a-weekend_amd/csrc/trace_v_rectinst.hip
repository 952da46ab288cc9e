// trace_v_rectinst.hip — instantiates the megakernel (trace_device.hpp) for one feature set
// (FEAT_SET_RECTINST, count_work false); each variant is its own translation unit so the build
// compiles them in parallel.
#include "trace_launch.hpp"

namespace rtk {
template hipError_t launch_variant<FEAT_SET_RECTINST, false>(const Launch&, const LaunchOpts&, hipStream_t);
}  // namespace rtk
