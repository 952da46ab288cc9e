// denoise_cross_host_main.cpp — rt_denoise_cross_host under ASan and UBSan
// (tests/test_denoise_cross_sanitized.py). Links csrc/cross_host.cpp alone: no HIP, nothing else of
// the library. Reads the cases the test wrote, runs each through rt_denoise_cross_host into buffers
// of exactly the frame's size and prints four checksums per case, in f64, in index order: sum_i out_i
// and sum_i (1 + i mod 7) out_i, and the same two of stderr_out.
//
// Input file: int32 n_cases, then per case int32 {width, height, format, radius, patch, guided},
// double k, double variance_scale, the two half means (height x width x 3 of the format), the error
// map (height x width f64) and, if guided, albedo, normal (height x width x 3 f64), depth (height x
// width f64) and the three sigmas (f64).
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
static int run_case(std::FILE* f, int index, const rt_cross_params& p, bool guided)
{
    const size_t hw = (size_t)p.width * (size_t)p.height;
    std::vector<T> a, b, out(3 * hw);
    std::vector<double> se, se_out(hw), albedo, normal, depth, sig;
    if (!read_n(f, a, 3 * hw) || !read_n(f, b, 3 * hw) || !read_n(f, se, hw)) return 2;
    rt_denoise_guides g{};
    if (guided) {
        if (!read_n(f, albedo, 3 * hw) || !read_n(f, normal, 3 * hw) || !read_n(f, depth, hw) || !read_n(f, sig, 3)) return 2;
        g = rt_denoise_guides{albedo.data(), normal.data(), depth.data(), sig[0], sig[1], sig[2]};
    }
    const int rc = rt_denoise_cross_host(&p, a.data(), b.data(), se.data(), guided ? &g : nullptr, out.data(), se_out.data());
    if (rc != RT_OK) {
        std::printf("case %d rc %d\n", index, rc);
        return 3;
    }
    // without stderr_out: the same frame, and nothing written through the null pointer
    std::vector<T> again(3 * hw);
    if (rt_denoise_cross_host(&p, a.data(), b.data(), se.data(), guided ? &g : nullptr, again.data(), nullptr) != RT_OK ||
        again != out)
        return 5;
    double s0, s1, e0, e1;
    sums(out, s0, s1);
    sums(se_out, e0, e1);
    std::printf("case %d %dx%d format %d r %d f %d sum %.17g weighted %.17g stderr %.17g weighted %.17g\n", index, p.width,
                p.height, p.format, p.radius, p.patch, s0, s1, e0, e1);
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
        int32_t h[6];
        double d[2];
        if (std::fread(h, sizeof h, 1, f) != 1 || std::fread(d, sizeof d, 1, f) != 1) {
            rc = 2;
            break;
        }
        rt_cross_params p{};
        p.width = h[0];
        p.height = h[1];
        p.format = h[2];
        p.radius = h[3];
        p.patch = h[4];
        p.k = d[0];
        p.variance_scale = d[1];
        rc = p.format == RT_OUT_F64 ? run_case<double>(f, i, p, h[5] != 0) : run_case<float>(f, i, p, h[5] != 0);
    }
    // the argument check, with pointers that must not be read
    rt_cross_params bad{};
    bad.width = bad.height = 4;
    bad.format = RT_OUT_F64;
    bad.radius = 11;
    bad.k = 0.45;
    bad.variance_scale = 2.0;
    double one[49] = {0};
    if (rc == 0 && rt_denoise_cross_host(&bad, one, one, one + 2, nullptr, one + 1, nullptr) != RT_ERR_INVALID) rc = 4;
    std::fclose(f);
    return rc;
}
