// pyramid_host_main.cpp — rt_denoise_pyramid_host under ASan and UBSan
// (tests/test_denoise_pyramid_sanitized.py). Links csrc/pyramid_host.cpp and csrc/denoise_host.cpp
// alone: no HIP, nothing else of the library. Reads the cases the test wrote, runs each through
// rt_denoise_pyramid_host with every buffer of exactly its frame's size and prints two checksums per
// case: sum_i x_i and sum_i (1 + i mod 7) x_i, in f64, in index order, of out.
//
// Input file: int32 n_cases, then per case int32 {width, height, format, radius, patch, levels, guide
// mask}, double {k, sigma_albedo, sigma_normal, sigma_depth}, the mean frame (height x width x 3 of
// the format), the error map (height x width f64) and the guides of the mask (bit 0 albedo, bit 1
// normal: height x width x 3 f64; bit 2 depth: height x width f64).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rt/rt_abi.h"

template <typename T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return std::fread(v.data(), sizeof(T), n, f) == n;
}

template <typename T>
static void sums(const std::vector<T>& v, double& s0, double& s1)
{
    s0 = s1 = 0.0;
    for (size_t i = 0; i < v.size(); ++i) {
        s0 = s0 + (double)v[i];
        s1 = s1 + (double)(1 + i % 7) * (double)v[i];
    }
}

template <typename T>
static int run_case(std::FILE* f, int index, const rt_pyramid_params& p, int mask, const double* sigma)
{
    const size_t hw = (size_t)p.width * (size_t)p.height;
    std::vector<T> mean, out(3 * hw);
    std::vector<double> se, albedo, normal, depth;
    if (!read_n(f, mean, 3 * hw) || !read_n(f, se, hw)) return 2;
    if ((mask & 1) && !read_n(f, albedo, 3 * hw)) return 2;
    if ((mask & 2) && !read_n(f, normal, 3 * hw)) return 2;
    if ((mask & 4) && !read_n(f, depth, hw)) return 2;
    rt_denoise_guides g{};
    g.albedo = (mask & 1) ? albedo.data() : nullptr;
    g.normal = (mask & 2) ? normal.data() : nullptr;
    g.depth = (mask & 4) ? depth.data() : nullptr;
    g.sigma_albedo = sigma[0];
    g.sigma_normal = sigma[1];
    g.sigma_depth = sigma[2];
    int rc = rt_denoise_pyramid_host(&p, mean.data(), se.data(), mask ? &g : nullptr, out.data());
    // a second call: the same frame
    std::vector<T> again(3 * hw);
    if (rc == RT_OK) rc = rt_denoise_pyramid_host(&p, mean.data(), se.data(), mask ? &g : nullptr, again.data());
    if (rc != RT_OK) {
        std::printf("case %d rc %d\n", index, rc);
        return 3;
    }
    for (size_t i = 0; i < out.size(); ++i)
        if (!(out[i] == again[i])) return 5;
    double s0, s1;
    sums(out, s0, s1);
    std::printf("case %d %dx%d format %d r %d f %d L %d guides %d sum %.17g weighted %.17g\n", index, p.width, p.height,
                p.format, p.radius, p.patch, p.levels, mask, s0, s1);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 1;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 1;
    int32_t n = 0;
    int rc = std::fread(&n, sizeof n, 1, f) == 1 ? 0 : 2;
    for (int i = 0; i < n && rc == 0; ++i) {
        int32_t h[7];
        double d[4];
        if (std::fread(h, sizeof h, 1, f) != 1 || std::fread(d, sizeof d, 1, f) != 1) {
            rc = 2;
            break;
        }
        rt_pyramid_params p{};
        p.width = h[0];
        p.height = h[1];
        p.format = h[2];
        p.radius = h[3];
        p.patch = h[4];
        p.levels = h[5];
        p.k = d[0];
        rc = p.format == RT_OUT_F64 ? run_case<double>(f, i, p, h[6], d + 1) : run_case<float>(f, i, p, h[6], d + 1);
    }
    // the argument check, with pointers that must not be read
    rt_pyramid_params ok{};
    ok.width = ok.height = 4;
    ok.format = RT_OUT_F64;
    ok.radius = 3;
    ok.patch = 1;
    ok.k = 0.45;
    ok.levels = 3;
    double one[49] = {0};
    rt_denoise_guides bad{};
    bad.depth = one;
    bad.sigma_depth = 0.0;
    if (rc == 0 && rt_denoise_pyramid_host(&ok, one, one, &bad, one + 1) != RT_ERR_INVALID) rc = 4;
    ok.levels = 6;
    if (rc == 0 && rt_denoise_pyramid_host(&ok, one, one, nullptr, one + 1) != RT_ERR_INVALID) rc = 4;
    ok.levels = 3;
    ok.reserved0 = 1;
    if (rc == 0 && rt_denoise_pyramid_host(&ok, one, one, nullptr, one + 1) != RT_ERR_INVALID) rc = 4;
    std::fclose(f);
    return rc;
}
