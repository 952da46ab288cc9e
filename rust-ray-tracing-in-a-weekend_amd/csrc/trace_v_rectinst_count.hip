// trace_v_rectinst_count.hip — instantiates the megakernel (trace_device.hpp) for one feature set
// (FEAT_SET_RECTINST, count_work true); each variant is its own translation unit so the build
// compiles them in parallel.
#include "trace_launch.hpp"

namespace rtk {
template hipError_t launch_variant<FEAT_SET_RECTINST, true>(const Launch&, const LaunchOpts&, hipStream_t);
}  // namespace rtk
