// camera_rays.cpp — rt_camera_rays (include/rt/rt_abi.h): the primary ray of every pixel's sample as
// rt_render shoots it, written out as rt_ray records. Host code without a context and without HIP:
// camera_begin, the unit-disk tries and camera_end of trace_shade.hpp restated over rt_numerics.h,
// operation for operation and in the kernel's association. The f64 kernels are built with
// contraction off and the numerics header is bit-identical on host and device, so these are the
// kernel's rays bit for bit (tests/test_gpu_trace_rays.py holds the device to it). The scales and
// reciprocals are camera_scales' (camera_rays.hpp), which the render driver puts into KParams.
#include <cmath>
#include <cstdint>
#include <string>

#include "rt/rt_abi.h"
#include "rt/rt_numerics.h"
#include "camera_rays.hpp"

namespace rtx {
int fail(int code, const std::string& msg);   // rt_last_error's slot (abi.cpp; a stand-alone program brings its own)
}

namespace {

// trace_types.hpp div_rcp: q / b through b's correctly rounded reciprocal y, RN(q / b) bit for bit
inline double div_rcp(double q, double b, double y)
{
    const double q0 = q * y;
    const double q1 = std::fma(std::fma(-b, q0, q), y, q0);
    if (q1 != q1) return q / b;
    return q1;
}

void camera_ray(const rt_camera& c, const rtc::CameraScales& k, int x, int y, int width, uint64_t seed, uint32_t sample,
                rt_ray& r)
{
    const uint32_t pixel = (uint32_t)y * (uint32_t)width + (uint32_t)x;
    rt_pstream st;
    rt_pstream_init(&st, seed, pixel, sample);
    // camera_begin: the pixel jitter
    const double u = div_rcp((double)x + rt_unit53(rt_pstream_u64(&st)), k.wm1, k.inv_wm1);
    const double v = div_rcp((double)y + rt_unit53(rt_pstream_u64(&st)), k.hm1, k.inv_hm1);
    // random_in_unit_disk: two draws per try (unit_try with z = 0: x*x + y*y + 0*0)
    double dxl, dyl;
    for (;;) {
        dxl = rt_uniform_sample(rt_pstream_u64(&st), -1.0, k.scale_m11);
        dyl = rt_uniform_sample(rt_pstream_u64(&st), -1.0, k.scale_m11);
        const double z = 0.0;
        if (dxl * dxl + dyl * dyl + z * z < 1.0) break;
    }
    // camera_end
    const double rdx = dxl * c.lens_radius, rdy = dyl * c.lens_radius;
    for (int a = 0; a < 3; ++a) {
        const double off = c.u[a] * rdx + c.v[a] * rdy;
        r.o[a] = c.origin[a] + off;
        r.d[a] = c.lower_left_corner[a] + c.horizontal[a] * u + c.vertical[a] * v - c.origin[a] - off;
    }
    r.time = rt_uniform_sample(rt_pstream_u64(&st), c.time0, k.scale_time);
    r.t_min = 0.001;
    r.t_max = RT_INF;
    r.key_pixel = pixel;
    r.key_sample = sample;
}

}  // namespace

extern "C" int rt_camera_rays(const rt_camera* cam, int width, int height, uint64_t render_seed, int sample, int tiled,
                              rt_ray* out)
{
    if (!cam || !out) return rtx::fail(RT_ERR_INVALID, "null argument");
    if (width < 2 || height < 2 || (long long)width * height > 0x7fffffffLL || sample < 0 || (tiled != 0 && tiled != 1))
        return rtx::fail(RT_ERR_INVALID, "rt_camera_rays: width, height >= 2, width * height <= 2^31 - 1, sample >= 0, tiled 0 or 1");
    const rtc::CameraScales k = rtc::camera_scales(*cam, width, height);
    size_t i = 0;
    if (!tiled) {
        for (int y = 0; y < height; ++y)
            for (int x = 0; x < width; ++x) camera_ray(*cam, k, x, y, width, render_seed, (uint32_t)sample, out[i++]);
        return RT_OK;
    }
    // the chunk kernels' lane order (trace_grid.hpp, lane_work): tile (ty, tx), lane = 8 * row + column
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    for (int ty = 0; ty < tiles_y; ++ty)
        for (int tx = 0; tx < tiles_x; ++tx)
            for (int lane = 0; lane < 64; ++lane) {
                const int x = tx * 8 + (lane & 7), y = ty * 8 + (lane >> 3);
                if (x < width && y < height) camera_ray(*cam, k, x, y, width, render_seed, (uint32_t)sample, out[i++]);
            }
    return RT_OK;
}
