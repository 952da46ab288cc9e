// sky_tiles_main.cpp — drives the host twin of the all-sky tile flags (csrc/primary_candidates_host.cpp,
// sky_tiles_host over csrc/primary_candidates.hpp's tile_all_sky) on the random scene, without HIP:
// links the scene builders, the flattener, the lowering and the host twin. For
// tests/test_sky_tiles.py, which also runs it under ASan and UBSan.
//
//   sky_tiles_main WIDTH HEIGHT K RAYS
//
// Builds scene 0 under its preset camera at WIDTH x HEIGHT, the candidate table with at most K
// candidates per pixel and the table's tile flags, and prints one JSON line: the tiles, the flagged
// ones, the pixels with an empty list, "mismatch" (tiles whose flag is not "every in-frame pixel
// has n == 0", recomputed here from the table) and "hits_in_sky": of RAYS rays per pixel of every
// flagged tile, drawn as the camera draws them (pixel jitter, lens disk, ray time; a generator of
// its own), how many hit any leaf primitive, brute force. Both must be 0.
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

// does the ray hit any sphere at t >= 0.001 (hittable.rs:254-273, MovingSphere::center)?
bool hits_any(const std::vector<rt_prim>& leaf, const double o[3], const double d[3], double time)
{
    const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    for (const rt_prim& p : leaf) {
        if (p.kind > RT_PRIM_MOVING_SPHERE) return true;   // (not a sphere: unknown, counted as a hit)
        double s = 0.0;
        if (p.kind == RT_PRIM_MOVING_SPHERE) s = (time - p.p[8]) / (p.p[9] - p.p[8]);
        const double oc[3] = {o[0] - (p.p[0] + p.p[5] * s), o[1] - (p.p[1] + p.p[6] * s), o[2] - (p.p[2] + p.p[7] * s)};
        const double half_b = oc[0] * d[0] + oc[1] * d[1] + oc[2] * d[2];
        const double c = oc[0] * oc[0] + oc[1] * oc[1] + oc[2] * oc[2] - p.p[3] * p.p[3];
        const double disc = half_b * half_b - a * c;
        if (disc < 0.0) continue;
        const double sq = std::sqrt(disc);
        if (!((-half_b - sq) / a < 0.001) || !((-half_b + sq) / a < 0.001)) return true;
    }
    return false;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s WIDTH HEIGHT K RAYS\n", argv[0]);
        return 2;
    }
    const int W = std::atoi(argv[1]), H = std::atoi(argv[2]), K = std::atoi(argv[3]), rays = std::atoi(argv[4]);
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
                                          0.1, 10.0, 0.0, 1.0);   // (rt_scene_camera's)

    std::vector<rtpc::Record> table((size_t)W * (size_t)H);
    rtpc::build_host(L.nodes.data(), L.leaf_prims.data(), w.flat.soa.tlas_root, cam, W, H, K, table.data());
    const int tx_n = rtpc::tiles_x_of(W), ty_n = rtpc::tiles_y_of(H);
    std::vector<uint8_t> flags((size_t)tx_n * (size_t)ty_n, 0xcc);
    const long long n_sky = (long long)rtpc::sky_tiles_host(table.data(), W, H, flags.data());

    long long empty_px = 0, mismatch = 0, counted = 0, hits = 0;
    for (size_t i = 0; i < table.size(); ++i) empty_px += table[i].n == 0;
    Rng rng{0x9E3779B97F4A7C15ull};
    for (int ty = 0; ty < ty_n; ++ty) {
        for (int tx = 0; tx < tx_n; ++tx) {
            bool all = true;
            for (int y = ty * 8; y < ty * 8 + 8 && y < H; ++y)
                for (int x = tx * 8; x < tx * 8 + 8 && x < W; ++x) all = all && table[(size_t)y * (size_t)W + (size_t)x].n == 0;
            const uint8_t f = flags[(size_t)ty * (size_t)tx_n + (size_t)tx];
            if (f != (all ? 1 : 0)) mismatch++;
            if (f != 1) continue;
            counted++;
            for (int y = ty * 8; y < ty * 8 + 8 && y < H; ++y) {
                for (int x = tx * 8; x < tx * 8 + 8 && x < W; ++x) {
                    for (int s = 0; s < rays; ++s) {
                        // (s 0..3: the pixel's corners, from the lens' rim)
                        const double ju = s < 4 ? (double)(s & 1) : rng.unit(), jv = s < 4 ? (double)(s >> 1) : rng.unit();
                        const double u = ((double)x + ju) / ((double)W - 1.0), v = ((double)y + jv) / ((double)H - 1.0);
                        double lx, ly;
                        do {
                            lx = 2.0 * rng.unit() - 1.0;
                            ly = 2.0 * rng.unit() - 1.0;
                        } while (lx * lx + ly * ly >= 1.0);
                        if (s < 4) lx = s & 1 ? 0.999999 : -0.999999, ly = 0.0;
                        const double rdx = lx * cam.lens_radius, rdy = ly * cam.lens_radius;
                        double o[3], d[3];
                        for (int a = 0; a < 3; ++a) {
                            const double off = cam.u[a] * rdx + cam.v[a] * rdy;
                            o[a] = cam.origin[a] + off;
                            d[a] = cam.lower_left_corner[a] + cam.horizontal[a] * u + cam.vertical[a] * v - cam.origin[a] - off;
                        }
                        const double time = cam.time0 + rng.unit() * (cam.time1 - cam.time0);
                        if (hits_any(L.leaf_prims, o, d, time)) hits++;
                    }
                }
            }
        }
    }
    if (counted != n_sky) mismatch++;
    std::printf("{\"width\": %d, \"height\": %d, \"k\": %d, \"tiles\": %d, \"sky_tiles\": %lld, \"empty_pixels\": %lld, "
                "\"mismatch\": %lld, \"rays\": %d, \"hits_in_sky\": %lld}\n",
                W, H, K, tx_n * ty_n, n_sky, empty_px, mismatch, rays, hits);
    return mismatch == 0 && hits == 0 ? 0 : 1;
}
