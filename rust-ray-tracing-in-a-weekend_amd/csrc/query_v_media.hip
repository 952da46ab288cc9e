// query_v_media.hip — instantiates rt_trace_rays' kernels (query_device.hpp) for one feature set
// (FEAT_SET_MEDIA); each variant is its own translation unit so the build compiles them in parallel.
#include "query_device.hpp"

namespace rtk {
template hipError_t launch_query_variant<FEAT_SET_MEDIA>(const SceneDev&, const QueryArgs&, int, const LaunchOpts&, hipStream_t);
}  // namespace rtk
