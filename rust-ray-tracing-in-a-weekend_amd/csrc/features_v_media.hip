// features_v_media.hip — instantiates rt_render_features' kernel (features_device.hpp) for one
// feature set (FEAT_SET_MEDIA); each variant is its own translation unit so the build compiles
// them in parallel.
#include "features_device.hpp"

namespace rtk {
template hipError_t launch_features_variant<FEAT_SET_MEDIA>(const Launch&, const LaunchOpts&, hipStream_t);
}  // namespace rtk
