// camera_rays.hpp — the host's statement of a frame's camera constants: the scales and reciprocals
// the primary ray of a (pixel, sample) is made with. The render driver copies them into the launch
// params (abi.cpp, fill_kparams -> KParams) and rt_camera_rays (camera_rays.cpp) makes the same rays
// with them on the host, so there is one statement of each. No HIP.
#pragma once

#include "rt/rt_numerics.h"
#include "rt/rt_scene.h"

namespace rtc {

struct CameraScales {
    double scale_m11;         // rand UniformFloat::new_inclusive(-1, 1) scale
    double scale_time;        // rand UniformFloat::new_inclusive(time0, time1) scale
    double wm1, hm1;          // width - 1, height - 1 (the jitter divisors of main.rs:517-518)
    double inv_wm1, inv_hm1;  // their reciprocals, correctly rounded
};

inline CameraScales camera_scales(const rt_camera& cam, int width, int height)
{
    CameraScales s;
    s.scale_m11 = rt_uniform_incl_scale(-1.0, 1.0);
    s.scale_time = rt_uniform_incl_scale(cam.time0, cam.time1);
    s.wm1 = (double)width - 1.0;
    s.hm1 = (double)height - 1.0;
    s.inv_wm1 = 1.0 / s.wm1;
    s.inv_hm1 = 1.0 / s.hm1;
    return s;
}

}  // namespace rtc
