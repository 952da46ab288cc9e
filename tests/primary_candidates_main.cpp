// primary_candidates_main.cpp — drives the host twin of the primary-candidate table
// (csrc/primary_candidates_host.cpp over csrc/primary_candidates.hpp) on the random scene, without
// HIP: links the scene builders, the flattener, the lowering and the host twin. For
// tests/test_primary_candidates.py, which also runs it under ASan and UBSan.
//
//   primary_candidates_main WIDTH HEIGHT K RAYS [APERTURE [TIME0 TIME1]]
//
// Builds scene 0 under its preset camera at WIDTH x HEIGHT, the table with at most K candidates per
// pixel, and prints one JSON line: the pixels, the flagged share, the candidate count's mean and
// max, and "contained": for RAYS rays per pixel drawn as the camera draws them (pixel jitter, lens
// disk, ray time; a generator of its own) the closest hit over every leaf primitive, brute force,
// is in the pixel's list or the pixel is flagged.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "primary_candidates.hpp"
#include "rt/rt_abi.h"
#include "scene_lower.hpp"
#include "scene_model.hpp"

namespace {

struct Rng {
    uint64_t s;
    double unit()   // [0, 1)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * 0x1.0p-53;
    }
};

// the closest hit of one ray over every leaf slot (hittable.rs:254-273, MovingSphere::center); -1: none
int closest(const std::vector<rt_prim>& leaf, const double o[3], const double d[3], double time)
{
    int best = -1;
    double t_max = INFINITY;
    const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    for (size_t j = 0; j < leaf.size(); ++j) {
        const rt_prim& p = leaf[j];
        if (p.kind > RT_PRIM_MOVING_SPHERE) continue;
        double s = 0.0;
        if (p.kind == RT_PRIM_MOVING_SPHERE) s = (time - p.p[8]) / (p.p[9] - p.p[8]);
        const double oc[3] = {o[0] - (p.p[0] + p.p[5] * s), o[1] - (p.p[1] + p.p[6] * s), o[2] - (p.p[2] + p.p[7] * s)};
        const double half_b = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2];
        const double c = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - p.p[3] * p.p[3];
        const double disc = half_b * half_b - a * c;
        if (disc < 0.0) continue;
        const double sq = std::sqrt(disc);
        double root = (-half_b - sq) / a;
        if (root < 0.001 || t_max < root) {
            root = (-half_b + sq) / a;
            if (root < 0.001 || t_max < root) continue;
        }
        t_max = root;
        best = (int)j;
    }
    return best;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s WIDTH HEIGHT K RAYS [APERTURE [TIME0 TIME1]]\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), K = std::atoi(argv[3]), rays = std::atoi(argv[4]);
    const double aperture = argc > 5 ? std::atof(argv[5]) : 0.1;
    const double time0 = argc > 7 ? std::atof(argv[6]) : 0.0, time1 = argc > 7 ? std::atof(argv[7]) : 1.0;
    if (W < 2 || H < 2 || K < 1 || rays < 0) return 2;

    rtw::World w(1);
    if (rtw::build_scene(w, 0, nullptr, 0, 0)) return 1;
    std::string err;
    if (rtw::flatten(w, RT_ACCEL_SAH, err)) {
        std::fprintf(stderr, "flatten: %s\n", err.c_str());
        return 1;
    }
    rtl::Lowered L;
    if (rtl::lower(w.flat.soa, true, L, err)) {
        std::fprintf(stderr, "lower: %s\n", err.c_str());
        return 1;
    }
    rtw::Preset pre;
    if (!rtw::scene_preset(0, pre)) return 1;
    const rt_camera cam = rtw::camera_new(pre.look_from, pre.look_at, rtw::v3(0.0, 1.0, 0.0), pre.vfov, (double)W / (double)H,
                                          aperture, 10.0, time0, time1);

    std::vector<rtpc::Record> table((size_t)W * (size_t)H);
    const rtpc::TableStats st = rtpc::build_host(L.nodes.data(), L.leaf_prims.data(), w.flat.soa.tlas_root, cam, W, H, K, table.data());

    Rng rng{0x9E3779B97F4A7C15ull};
    long long outside = 0, hits = 0;
    for (int y = 0; y < H; ++y) {
        for (int x = 0; x < W; ++x) {
            const rtpc::Record& r = table[(size_t)y * (size_t)W + (size_t)x];
            for (int s = 0; s < rays; ++s) {
                const double u = ((double)x + rng.unit()) / ((double)W - 1.0), v = ((double)y + rng.unit()) / ((double)H - 1.0);
                double lx, ly;
                do {
                    lx = 2.0 * rng.unit() - 1.0;
                    ly = 2.0 * rng.unit() - 1.0;
                } while (lx * lx + ly * ly >= 1.0);
                if (s == 0) lx = 0.999999, ly = 0.0;   // the lens' rim
                const double rdx = lx * cam.lens_radius, rdy = ly * cam.lens_radius;
                double o[3], d[3];
                for (int a = 0; a < 3; ++a) {
                    const double off = cam.u[a] * rdx + cam.v[a] * rdy;
                    o[a] = cam.origin[a] + off;
                    d[a] = cam.lower_left_corner[a] + cam.horizontal[a] * u + cam.vertical[a] * v - cam.origin[a] - off;
                }
                const double time = cam.time0 + rng.unit() * (cam.time1 - cam.time0);
                const int hit = closest(L.leaf_prims, o, d, time);
                if (hit < 0) continue;
                hits++;
                if (r.n == rtpc::kWalk) continue;
                bool in = false;
                for (int i = 0; i < (int)r.n; ++i) in = in || (int)r.slot[i] == hit;
                if (!in) outside++;
            }
        }
    }
    const long long listed = st.pixels - st.flagged;
    std::printf("{\"width\": %d, \"height\": %d, \"k\": %d, \"pixels\": %lld, \"flagged\": %lld, \"flagged_share\": %.6f, "
                "\"mean_candidates\": %.4f, \"max_candidates\": %d, \"table_bytes\": %zu, \"rays\": %lld, \"hits\": %lld, "
                "\"outside\": %lld, \"contained\": %s}\n",
                W, H, K, (long long)st.pixels, (long long)st.flagged, (double)st.flagged / (double)st.pixels,
                listed ? (double)st.candidates / (double)listed : 0.0, st.max_candidates, rtpc::table_bytes(W, H),
                (long long)rays * W * H, hits, outside, outside == 0 ? "true" : "false");
    return outside == 0 ? 0 : 1;
}
