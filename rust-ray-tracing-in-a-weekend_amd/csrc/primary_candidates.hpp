// primary_candidates.hpp — which primitives a pixel's primary rays can hit, decided once per
// (scene upload, camera, frame size) so that a new sample of the f64 spheres pool kernel takes its
// first hit from a short exact test of its pixel's candidates instead of a walk.
//
// Every primary ray of pixel (ix, y) is (1 - t) L + t T: L on the lens (within lens_radius of the
// camera's origin O in the plane of cam.u, cam.v), T in the pixel's parallelogram of the focus
// plane, whatever the jitter, the lens point and the ray time. With T0 the parallelogram's centre
// the ray stays within R(t) = |1 - t| lr + t hd of the axis A(t) = (1 - t) O + t T0 (lr: the lens
// radius as a length, hd: the parallelogram's half diagonal): a thin double cone. A sphere (centre
// c, radius rho) can be hit only if |A(t) - c| <= |rho| + R(t) for some t >= 0. R changes by at most
// (lr + hd) per unit t and A moves |T0 - O| per unit t, so with t* the axis parameter nearest to c
// (clamped to t >= 0) and k = (lr + hd) / |T0 - O| < 1 that needs
//     |A(t*) - c| sqrt(1 - k^2) <= |rho| + R(t*),
// which is the test below, with an outward margin for the f64 rounding of the ray arithmetic.
// A moving sphere is tested against its swept bound over the camera's shutter (the segment of its
// centres in pieces, a ball around each); any other primitive kind is "unknown", and its pixel
// keeps the walk.
//
// No HIP: the table kernel (primary_candidates.hip), the host twin (primary_candidates_host.cpp)
// and tests/primary_candidates_main.cpp run the same build_pixel.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt/rt_scene.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RT_PC_HD __host__ __device__ inline
#else
#define RT_PC_HD inline
#endif

namespace rtpc {

// A pixel's record, 16 bytes: n candidates (leaf slots of the TLAS, in walk order), or kWalk
constexpr int kSlots = 7;
constexpr uint16_t kWalk = 0xffff;
struct Record {   // (the device table is 16-byte aligned: one load)
    uint16_t n;
    uint16_t slot[kSlots];
};
static_assert(sizeof(Record) == 16, "one 16-byte load per new sample");

// The table is skipped (the render walks as before) beyond this many bytes: 256 MiB, 16.7 M pixels
// (a 7680 x 2160 frame: 253 MiB)
constexpr size_t kMaxTableBytes = (size_t)256 << 20;
// and the cone is "not covered" beyond this k (the bound needs k < 1; a camera this wide per pixel,
// or focused this close to its lens, gains nothing from a list anyway)
constexpr double kMaxSlope = 0.5;
// pieces a moving sphere's sweep over the shutter is tested in, at most
constexpr int kSweepPieces = 32;
// walk stack of build_pixel (a TLAS needs at most 32 entries, rt_scene_soa.tlas_depth)
constexpr int kStack = 64;

struct Cone {
    double o[3], d[3];   // the axis: O + t (T0 - O)
    double dd;           // |T0 - O|^2
    double lr, hd;       // lens radius and pixel half diagonal, as lengths
    double shrink;       // sqrt(1 - k^2)
    double time_lo, time_hi;   // the camera's shutter, ordered
    bool covered;        // false: the bound does not hold for this camera, every pixel walks
};

RT_PC_HD double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
RT_PC_HD bool is_fin(double x) { return x - x == 0.0; }

// the cone of image pixel (ix, y) (row 0 = bottom: camera_begin's u = (ix + xi) / (W - 1), v = (y + xi) / (H - 1))
RT_PC_HD Cone cone_of(const rt_camera& cam, int width, int height, int ix, int y)
{
    Cone c;
    const double su = ((double)ix + 0.5) / ((double)width - 1.0), sv = ((double)y + 0.5) / ((double)height - 1.0);
    double hh = 0.0, vv = 0.0;
    for (int a = 0; a < 3; ++a) {
        c.o[a] = cam.origin[a];
        c.d[a] = cam.lower_left_corner[a] + cam.horizontal[a] * su + cam.vertical[a] * sv - cam.origin[a];
        hh += cam.horizontal[a] * cam.horizontal[a];
        vv += cam.vertical[a] * cam.vertical[a];
    }
    c.dd = dot3(c.d, c.d);
    c.hd = 0.5 * (__builtin_sqrt(hh) / ((double)width - 1.0) + __builtin_sqrt(vv) / ((double)height - 1.0));
    // |u a + v b| <= sigma_max([u v]) |(a, b)|, sigma_max^2 <= max(|u|^2, |v|^2) + |u . v|
    const double uu = dot3(cam.u, cam.u), vv2 = dot3(cam.v, cam.v), uv = __builtin_fabs(dot3(cam.u, cam.v));
    c.lr = __builtin_fabs(cam.lens_radius) * __builtin_sqrt((uu > vv2 ? uu : vv2) + uv);
    c.time_lo = cam.time0 < cam.time1 ? cam.time0 : cam.time1;
    c.time_hi = cam.time0 < cam.time1 ? cam.time1 : cam.time0;
    const double k = (c.lr + c.hd) / __builtin_sqrt(c.dd);
    c.covered = width > 1 && height > 1 && c.dd > 0.0 && is_fin(c.dd) && is_fin(c.lr) && is_fin(c.hd) && k <= kMaxSlope &&
                is_fin(c.time_lo) && is_fin(c.time_hi);
    c.shrink = c.covered ? __builtin_sqrt(1.0 - k * k) : 0.0;
    return c;
}

// may a ray of the cone meet the ball (centre, radius >= 0)? Anything not finite: yes.
RT_PC_HD bool may_hit_ball(const Cone& c, const double* centre, double radius)
{
    const double w[3] = {centre[0] - c.o[0], centre[1] - c.o[1], centre[2] - c.o[2]};
    double t = dot3(w, c.d) / c.dd;
    if (!(t > 0.0)) t = 0.0;
    const double q[3] = {w[0] - t * c.d[0], w[1] - t * c.d[1], w[2] - t * c.d[2]};
    const double dist = __builtin_sqrt(dot3(q, q));
    const double cone_r = __builtin_fabs(1.0 - t) * c.lr + t * c.hd;
    const double reach = radius + cone_r;
    const double margin = 1e-7 * (1.0 + reach + dist);
    return !(dist * c.shrink > reach + margin);   // (a NaN compares false: "may")
}

enum Verdict { kMiss = 0, kMay = 1, kUnknown = 2 };

// a leaf primitive (soa or device record: a Sphere's velocity is read only for a MovingSphere)
RT_PC_HD Verdict may_hit_prim(const Cone& c, const rt_prim& p)
{
    const double rho = __builtin_fabs(p.p[3]);
    if (p.kind == RT_PRIM_SPHERE) return may_hit_ball(c, p.p, rho) ? kMay : kMiss;
    if (p.kind != RT_PRIM_MOVING_SPHERE) return kUnknown;
    // MovingSphere::center over the shutter: c0 + s (c1 - c0), s = time, or (time - t0) / (t1 - t0)
    double s0 = c.time_lo, s1 = c.time_hi;
    if (!(p.p[8] == 0.0 && p.p[9] == 1.0)) {
        s0 = (c.time_lo - p.p[8]) / (p.p[9] - p.p[8]);
        s1 = (c.time_hi - p.p[8]) / (p.p[9] - p.p[8]);
    }
    // the centres' segment in pieces, each bounded by the ball around it: as many as keep a piece's
    // half length under a quarter of the radius (at most kSweepPieces; one piece for a sphere at rest)
    const double speed = __builtin_sqrt(p.p[5] * p.p[5] + p.p[6] * p.p[6] + p.p[7] * p.p[7]);
    const double half = 0.5 * __builtin_fabs(s1 - s0) * speed;
    if (!is_fin(half) || !is_fin(s0) || !is_fin(s1)) return kMay;
    int pieces = 1;
    while (pieces < kSweepPieces && half > 0.25 * rho * (double)pieces) pieces *= 2;
    const double ds = (s1 - s0) / (double)pieces, piece = half / (double)pieces;
    for (int i = 0; i < pieces; ++i) {
        const double sm = s0 + ((double)i + 0.5) * ds;
        const double mid[3] = {p.p[0] + p.p[5] * sm, p.p[1] + p.p[6] * sm, p.p[2] + p.p[7] * sm};
        if (may_hit_ball(c, mid, rho + piece + 1e-9 * (1.0 + piece + half))) return kMay;
    }
    return kMiss;
}

// a node's child box, as the ball around it (the cone fattened into the slab test; an unbounded box: yes)
RT_PC_HD bool may_hit_box(const Cone& c, const float* lo, const float* hi)
{
    double mid[3], h2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        mid[a] = 0.5 * ((double)lo[a] + (double)hi[a]);
        const double h = 0.5 * ((double)hi[a] - (double)lo[a]);
        h2 += h * h;
    }
    if (!is_fin(h2) || !is_fin(mid[0]) || !is_fin(mid[1]) || !is_fin(mid[2])) return true;
    return may_hit_ball(c, mid, __builtin_sqrt(h2));
}

// One pixel's record: the TLAS (nodes, root reference, records in leaf-slot order) walked with the
// cone. k_max <= kSlots: more candidates than that flag the pixel (the test hook forces 1).
RT_PC_HD Record build_pixel(const rt_bvh_node* nodes, const rt_prim* leaf_prims, int32_t root, const Cone& c, int k_max)
{
    Record r;
    r.n = 0;
    for (int i = 0; i < kSlots; ++i) r.slot[i] = 0;
    if (!c.covered) {
        r.n = kWalk;
        return r;
    }
    int32_t stack[kStack];
    int sp = 0;
    int32_t cur = root;
    for (;;) {
        if (cur >= 0) {
            const rt_bvh_node& nd = nodes[cur];
            const bool h0 = may_hit_box(c, nd.lo0, nd.hi0), h1 = may_hit_box(c, nd.lo1, nd.hi1);
            if (h0 && h1) {
                if (sp == kStack) {
                    r.n = kWalk;
                    return r;
                }
                stack[sp++] = nd.child[1];
                cur = nd.child[0];
                continue;
            }
            if (h0 || h1) {
                cur = h0 ? nd.child[0] : nd.child[1];
                continue;
            }
        } else {
            const int32_t code = ~cur, first = code >> 5, count = cur == INT32_MIN ? 0 : code & 31;   // (INT32_MIN: an empty BVH)
            for (int32_t j = first; j < first + count; ++j) {
                const Verdict v = may_hit_prim(c, leaf_prims[j]);
                if (v == kMiss) continue;
                if (v == kUnknown || (int)r.n >= k_max || j >= (int32_t)kWalk) {
                    r.n = kWalk;
                    return r;
                }
                r.slot[r.n++] = (uint16_t)j;
            }
        }
        if (sp == 0) return r;
        cur = stack[--sp];
    }
}

// ---- all-sky tiles (RT_OPT_SKIP_SKY_TILES) --------------------------------------------------------
// A pixel listed with n == 0 has no primitive any of its primary rays can meet: at max_depth >= 1
// every sample of it is 0.0 + 1.0 * background, whatever its draws. An 8x8 raster tile (tx, ty) of
// the frame whose in-frame pixels are all listed so is never dealt to the trace kernel; the
// reduction sums that constant in the records' place. A flagged pixel (kWalk) is
// not sky.
RT_PC_HD int tiles_x_of(int width) { return (width + 7) / 8; }
RT_PC_HD int tiles_y_of(int height) { return (height + 7) / 8; }
RT_PC_HD bool tile_all_sky(const Record* table, int width, int height, int tx, int ty)
{
    const int x1 = tx * 8 + 8 < width ? tx * 8 + 8 : width, y1 = ty * 8 + 8 < height ? ty * 8 + 8 : height;
    for (int y = ty * 8; y < y1; ++y)
        for (int x = tx * 8; x < x1; ++x)
            if (table[(size_t)y * (size_t)width + (size_t)x].n != 0) return false;
    return true;
}

// ---- the host twin (primary_candidates_host.cpp) ------------------------------------------------
struct TableStats {
    int64_t pixels = 0, flagged = 0, candidates = 0;   // candidates: summed over the pixels not flagged
    int max_candidates = 0;
};
// out[y * width + ix], row 0 = bottom
TableStats build_host(const rt_bvh_node* nodes, const rt_prim* leaf_prims, int32_t root, const rt_camera& cam, int width,
                      int height, int k_max, Record* out);
inline size_t table_bytes(int width, int height) { return (size_t)width * (size_t)height * sizeof(Record); }
// the all-sky flags of a table, flags[ty * tiles_x_of(width) + tx] = 1 or 0; returns how many are set
int64_t sky_tiles_host(const Record* table, int width, int height, uint8_t* flags);

}  // namespace rtpc
