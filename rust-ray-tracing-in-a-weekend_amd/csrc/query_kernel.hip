// query_kernel.hip — host-side dispatch of rt_trace_rays' trace_query variants (query_v_*.hip over
// query_device.hpp).
#include "query_device.hpp"

namespace rtk {

hipError_t launch_query(const SceneDev& S, const QueryArgs& Q, int mode, const LaunchOpts& o, hipStream_t stream)
{
    if (o.f32 || o.count) return hipErrorNotSupported;
    if (mode != RT_QUERY_CLOSEST && mode != RT_QUERY_ANY) return hipErrorInvalidValue;
    if (Q.n == 0) return hipSuccess;
    if (Q.n < 0 || Q.n > 0x7fffffffLL) return hipErrorInvalidValue;
    const uint32_t f = variant_features(o.features);
    if (f == FEAT_SET_SPHERES) return launch_query_variant<FEAT_SET_SPHERES>(S, Q, mode, o, stream);
    if (f == FEAT_SET_RECTINST) return launch_query_variant<FEAT_SET_RECTINST>(S, Q, mode, o, stream);
    if (f == FEAT_SET_MEDIA) return launch_query_variant<FEAT_SET_MEDIA>(S, Q, mode, o, stream);
    if (f == FEAT_SET_FINAL) return launch_query_variant<FEAT_SET_FINAL>(S, Q, mode, o, stream);
    return launch_query_variant<FEAT_ALL>(S, Q, mode, o, stream);
}

}  // namespace rtk
