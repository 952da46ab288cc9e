// camera_rays_main.cpp — drives rt_camera_rays (csrc/camera_rays.cpp) on its own, without HIP and
// without the library: links that one source. For tests/test_camera_rays.py, which builds it with
// ASan and UBSan, runs it directly and compares the records it dumps with the library's.
//
//   camera_rays_main CAMERA_FILE OUT_FILE SEED WIDTH HEIGHT SAMPLE TILED [WIDTH HEIGHT SAMPLE TILED ...]
//
// CAMERA_FILE holds an rt_camera (24 doubles). For every (WIDTH, HEIGHT, SAMPLE, TILED) it calls
// rt_camera_rays into a buffer of exactly width * height records and appends them to OUT_FILE.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "rt/rt_abi.h"

namespace rtx {
int fail(int code, const std::string& msg)   // the library's rt_last_error slot, here stderr
{
    std::fprintf(stderr, "rt error %d: %s\n", code, msg.c_str());
    return code;
}
}  // namespace rtx

int main(int argc, char** argv)
{
    if (argc < 8 || (argc - 4) % 4 != 0) {
        std::fprintf(stderr, "usage: %s CAMERA_FILE OUT_FILE SEED WIDTH HEIGHT SAMPLE TILED [...]\n", argv[0]);
        return 2;
    }
    static_assert(sizeof(rt_camera) == 24 * sizeof(double) && sizeof(rt_ray) == 80 && sizeof(rt_hit) == 80, "record sizes");
    rt_camera cam;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(&cam, sizeof cam, 1, f) != 1) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    std::fclose(f);
    std::FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 1;
    const uint64_t seed = std::strtoull(argv[3], nullptr, 10);
    for (int a = 4; a + 3 < argc; a += 4) {
        const int W = std::atoi(argv[a]), H = std::atoi(argv[a + 1]), sample = std::atoi(argv[a + 2]), tiled = std::atoi(argv[a + 3]);
        if (W < 2 || H < 2) return 2;
        std::vector<rt_ray> rays((size_t)W * (size_t)H);
        if (rt_camera_rays(&cam, W, H, seed, sample, tiled, rays.data()) != RT_OK) return 1;
        if (std::fwrite(rays.data(), sizeof(rt_ray), rays.size(), out) != rays.size()) return 1;
    }
    // the argument checks: each refused, nothing written
    rt_ray one[4];
    if (rt_camera_rays(nullptr, 2, 2, seed, 0, 0, one) != RT_ERR_INVALID || rt_camera_rays(&cam, 1, 2, seed, 0, 0, one) != RT_ERR_INVALID ||
        rt_camera_rays(&cam, 2, 2, seed, -1, 0, one) != RT_ERR_INVALID || rt_camera_rays(&cam, 2, 2, seed, 0, 2, one) != RT_ERR_INVALID)
        return 3;
    return std::fclose(out) == 0 ? 0 : 1;
}
