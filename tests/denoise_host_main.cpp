// denoise_host_main.cpp — rt_denoise_host under ASan and UBSan (tests/test_denoise_sanitized.py).
// Links csrc/denoise_host.cpp alone: no HIP, nothing else of the library. Reads the cases the
// test wrote, runs each through rt_denoise_host into a buffer of exactly the frame's size and
// prints two checksums per case: sum_i out_i and sum_i (1 + i mod 7) out_i, in f64, in index order.
//
// Input file: int32 n_cases, then per case int32 {width, height, format, radius, patch}, double k,
// the mean frame (height x width x 3 of the format) and the error map (height x width f64).
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
static int run_case(std::FILE* f, int index, const rt_denoise_params& p)
{
    const size_t hw = (size_t)p.width * (size_t)p.height;
    std::vector<T> mean, out(3 * hw);
    std::vector<double> se;
    if (!read_n(f, mean, 3 * hw) || !read_n(f, se, hw)) return 2;
    const int rc = rt_denoise_host(&p, mean.data(), se.data(), out.data());
    if (rc != RT_OK) {
        std::printf("case %d rc %d\n", index, rc);
        return 3;
    }
    double s0 = 0.0, s1 = 0.0;
    for (size_t i = 0; i < out.size(); ++i) {
        s0 = s0 + (double)out[i];
        s1 = s1 + (double)(1 + i % 7) * (double)out[i];
    }
    std::printf("case %d %dx%d format %d r %d f %d sum %.17g weighted %.17g\n", index, p.width, p.height, p.format,
                p.radius, p.patch, s0, s1);
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
        int32_t h[5];
        double k = 0.0;
        if (std::fread(h, sizeof h, 1, f) != 1 || std::fread(&k, sizeof k, 1, f) != 1) {
            rc = 2;
            break;
        }
        rt_denoise_params p{};
        p.width = h[0];
        p.height = h[1];
        p.format = h[2];
        p.radius = h[3];
        p.patch = h[4];
        p.k = k;
        rc = p.format == RT_OUT_F64 ? run_case<double>(f, i, p) : run_case<float>(f, i, p);
    }
    // the argument check, with pointers that must not be read
    rt_denoise_params bad{};
    bad.width = bad.height = 4;
    bad.format = RT_OUT_F64;
    bad.radius = 11;
    bad.k = 0.45;
    double one[48] = {0};
    if (rc == 0 && rt_denoise_host(&bad, one, one, one + 1) != RT_ERR_INVALID) rc = 4;
    std::fclose(f);
    return rc;
}
