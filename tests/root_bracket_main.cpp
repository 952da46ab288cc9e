// root_bracket_main.cpp — drives csrc/root_bracket.hpp (RT_OPT_DEFER_ROOTS) on the host, without HIP:
// the f32 brackets against sphere_t's own f64 roots, and a host twin of the deferred closest-hit loop
// against the sequential exact loop of the walk's do_leaf. For tests/test_root_bracket.py, which
// also runs it under ASan and UBSan.
//
//   root_bracket_main RANDOM_INPUTS SCENE_RAYS
//
// Prints one JSON line and exits 0 only if nothing failed:
//   containment: for RANDOM_INPUTS random (half_b, disc, |d|^2) — half of them from random rays and
//     spheres (r = 1000, 1, 0.2 and 1e-3, origins on the surface included, |d|^2 from 2^-60 to 2^60),
//     half log-uniform over wide exponent ranges — plus the constructed ones (disc 0, one ulp, 1e-300;
//     |d|^2 outside div_rcp's guard; infinite and NaN direction components), `roots` either reports
//     "outside the premises" or both brackets hold the computed f64 roots strictly ("violations").
//   equivalence: on every world and ray below, in forward, reverse and 20 shuffled test orders, the
//     deferred loop returns the sequential loop's (slot, t bits) ("mismatches"): scene 0's spheres
//     with SCENE_RAYS bounce-like rays (origin on a sphere's surface, direction its normal plus a
//     random unit-ball vector, unnormalised); two identical spheres; centres 1 ulp, 1e-12 and 1e-7
//     apart; rays that meet NaN.
//   fallback share: of the scene-0 tests with disc >= 0, how many `closer` decided exactly.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "root_bracket.hpp"
#include "rt/rt_abi.h"
#include "scene_lower.hpp"
#include "scene_model.hpp"

namespace {

constexpr double kInf = std::numeric_limits<double>::infinity();
constexpr double kNaN = std::numeric_limits<double>::quiet_NaN();

struct Rng {
    uint64_t s;
    double unit()   // [0, 1)
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * 0x1.0p-53;
    }
    double sym() { return 2.0 * unit() - 1.0; }
    void in_ball(double v[3])
    {
        do {
            for (int a = 0; a < 3; ++a) v[a] = sym();
        } while (v[0] * v[0] + v[1] * v[1] + v[2] * v[2] >= 1.0);
    }
    void on_sphere(double v[3])
    {
        double l2;
        do {
            in_ball(v);
            l2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        } while (l2 < 1e-4);
        const double l = std::sqrt(l2);
        for (int a = 0; a < 3; ++a) v[a] /= l;
    }
};

// ---- the kernel's f64 arithmetic, restated (trace_types.hpp rcp_for_div / div_rcp, trace_prims.hpp
// sphere_t, sphere_quad, sphere_root, sphere_center)
struct Ray {
    double o[3], d[3], time, a, ya;
};
double rcp_for_div(double b)
{
    const double m = std::fabs(b);
    return (m >= 0x1.0p-900 && m <= 0x1.0p+900) ? 1.0 / b : kNaN;
}
double div_rcp(double q, double b, double y)
{
    const double q0 = q * y;
    const double q1 = std::fma(std::fma(-b, q0, q), y, q0);
    if (q1 != q1) return q / b;
    return q1;
}
void finish_ray(Ray& r)
{
    r.a = r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2];
    r.ya = rcp_for_div(r.a);
}
struct Sphere {
    double c0[3], v[3], radius;   // centre c0 + v * time
};
void quad(const Sphere& s, const Ray& r, double& half_b, double& disc)
{
    const double cx = s.c0[0] + s.v[0] * r.time, cy = s.c0[1] + s.v[1] * r.time, cz = s.c0[2] + s.v[2] * r.time;
    const double ocx = r.o[0] - cx, ocy = r.o[1] - cy, ocz = r.o[2] - cz;
    half_b = ocx * r.d[0] + ocy * r.d[1] + ocz * r.d[2];
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - s.radius * s.radius;
    disc = half_b * half_b - r.a * c;
}
bool sphere_t(const Sphere& s, const Ray& r, double t_min, double t_max, double& t)
{
    double half_b, disc;
    quad(s, r, half_b, disc);
    if (disc < 0.0) return false;
    const double sqrtd = std::sqrt(disc);
    double root = div_rcp(-half_b - sqrtd, r.a, r.ya);
    if (root < t_min || t_max < root) {
        root = div_rcp(-half_b + sqrtd, r.a, r.ya);
        if (root < t_min || t_max < root) return false;
    }
    t = root;
    return true;
}
bool sphere_root(double half_b, double disc, const Ray& r, double t_min, double& t)
{
    const double sqrtd = std::sqrt(disc);
    double root = div_rcp(-half_b - sqrtd, r.a, r.ya);
    if (root < t_min) {
        root = div_rcp(-half_b + sqrtd, r.a, r.ya);
        if (root < t_min) return false;
    }
    t = root;
    return true;
}

// ---- containment ------------------------------------------------------------------------------
struct Contain {
    long long inputs = 0, valid = 0, ambiguous = 0, violations = 0;
    long long plain = 0, plain_valid = 0;   // everyday inputs (random-scene-like), which must not be ambiguous
    double worst = 0.0;   // max |root - bracket centre| / bracket half width over the valid ones
};
void contain(double half_b, double disc, double a, Contain& c, bool plain = false)
{
    if (disc < 0.0) return;   // (sphere_t returns before the roots)
    c.inputs++;
    c.plain += plain;
    const double ya = rcp_for_div(a);
    const double sqrtd = std::sqrt(disc);
    const double near = div_rcp(-half_b - sqrtd, a, ya), far = div_rcp(-half_b + sqrtd, a, ya);
    float nlo, nhi, flo, fhi;
    if (!rtrb::roots(half_b, disc, rtrb::ya32(ya), nlo, nhi, flo, fhi)) {
        c.ambiguous++;
        return;
    }
    c.valid++;
    c.plain_valid += plain;
    if (!((double)nlo < near && near < (double)nhi && (double)flo < far && far < (double)fhi)) {
        if (c.violations++ < 5)
            std::fprintf(stderr, "violation: half_b %a disc %a a %a: near %a in [%a, %a], far %a in [%a, %a]\n", half_b, disc, a,
                         near, (double)nlo, (double)nhi, far, (double)flo, (double)fhi);
        return;
    }
    const double hw = 0.5 * ((double)nhi - (double)nlo), mid = 0.5 * ((double)nhi + (double)nlo);
    if (hw > 0.0) c.worst = std::fmax(c.worst, std::fabs(near - mid) / hw);
    const double hwf = 0.5 * ((double)fhi - (double)flo), midf = 0.5 * ((double)fhi + (double)flo);
    if (hwf > 0.0) c.worst = std::fmax(c.worst, std::fabs(far - midf) / hwf);
}
void contain_ray(const Sphere& s, Ray r, Contain& c, bool plain = false)
{
    finish_ray(r);
    double half_b, disc;
    quad(s, r, half_b, disc);
    contain(half_b, disc, r.a, c, plain);
}

// ---- the two loops ----------------------------------------------------------------------------
bool sequential(const std::vector<Sphere>& w, const std::vector<int>& order, const Ray& r, int& slot, double& t)
{
    double t_max = kInf;
    bool any = false;
    for (int i : order) {
        double tt;
        if (sphere_t(w[(size_t)i], r, 0.001, t_max, tt)) {
            slot = i;
            t_max = tt;
            any = true;
        }
    }
    t = t_max;
    return any;
}
bool deferred(const std::vector<Sphere>& w, const std::vector<int>& order, const Ray& r, int& slot, double& t, rtrb::Tally& tally)
{
    const double t_min = 0.001;
    auto exact_of = [&](int s, double& tt) {
        double hb, disc;
        quad(w[(size_t)s], r, hb, disc);
        if (disc < 0.0) return false;
        return sphere_root(hb, disc, r, t_min, tt);
    };
    rtrb::Best best = rtrb::none();
    for (int i : order) {
        double half_b, disc;
        quad(w[(size_t)i], r, half_b, disc);
        if (disc < 0.0) continue;
        (void)rtrb::closer(
            best, i, half_b, disc, rtrb::ya32(r.ya), rtrb::down(t_min), rtrb::up(t_min),
            [&](double& tt) { return sphere_root(half_b, disc, r, t_min, tt); }, exact_of, &tally);
    }
    if (best.prim < 0) return false;
    slot = best.prim;
    return exact_of(best.prim, t);
}
struct Equiv {
    long long rays = 0, casts = 0, hits = 0, mismatches = 0;
};
void compare(const std::vector<Sphere>& w, Ray r, Rng& rng, Equiv& e, rtrb::Tally& tally)
{
    finish_ray(r);
    e.rays++;
    const int n = (int)w.size();
    std::vector<int> order((size_t)n);
    for (int k = 0; k < 22; ++k) {
        for (int i = 0; i < n; ++i) order[(size_t)i] = k == 1 ? n - 1 - i : i;
        if (k >= 2)
            for (int i = n - 1; i > 0; --i) std::swap(order[(size_t)i], order[(size_t)(rng.unit() * (i + 1))]);
        int s0 = -1, s1 = -1;
        double t0 = 0.0, t1 = 0.0;
        const bool h0 = sequential(w, order, r, s0, t0), h1 = deferred(w, order, r, s1, t1, tally);
        e.casts++;
        e.hits += h0;
        if (h0 != h1 || (h0 && (s0 != s1 || std::memcmp(&t0, &t1, sizeof t0) != 0))) {
            if (e.mismatches++ < 5)
                std::fprintf(stderr, "mismatch (order %d): sequential %d slot %d t %a, deferred %d slot %d t %a\n", k, (int)h0, s0,
                             t0, (int)h1, s1, t1);
        }
    }
}
// a bounce-like ray off sphere s: origin on its surface, direction the normal plus a unit-ball vector
Ray bounce_ray(const Sphere& s, Rng& rng)
{
    Ray r{};
    r.time = rng.unit();
    double n[3], b[3];
    rng.on_sphere(n);
    rng.in_ball(b);
    for (int a = 0; a < 3; ++a) {
        r.o[a] = s.c0[a] + s.v[a] * r.time + s.radius * n[a];
        r.d[a] = n[a] + b[a];
    }
    return r;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s RANDOM_INPUTS SCENE_RAYS\n", argv[0]);
        return 2;
    }
    const long long n_random = std::atoll(argv[1]);
    const int n_rays = std::atoi(argv[2]);
    Rng rng{0x243F6A8885A308D3ull};

    // ---- containment: random ------------------------------------------------------------------
    Contain c;
    const double radii[4] = {1000.0, 1.0, 0.2, 1e-3};
    for (long long i = 0; i < n_random / 2; ++i) {
        Sphere s{};
        s.radius = radii[i & 3];
        for (int a = 0; a < 3; ++a) s.c0[a] = 12.0 * rng.sym();
        if (s.radius == 1000.0) s.c0[1] = -1000.0;
        Ray r{};
        double n[3], b[3];
        rng.on_sphere(n);
        rng.in_ball(b);
        const bool surface = (i >> 2 & 1) != 0;   // the origin on this sphere's surface, or anywhere near the scene
        const double scale = (i >> 3 & 1) ? std::ldexp(1.0, (int)(rng.unit() * 61.0) - 30) : 1.0;   // |d|^2 2^-60 .. 2^60
        for (int a = 0; a < 3; ++a) {
            r.o[a] = surface ? s.c0[a] + s.radius * n[a] : 14.0 * rng.sym();
            r.d[a] = (surface ? n[a] + b[a] : (s.c0[a] + s.radius * b[a]) - r.o[a]) * scale;
        }
        contain_ray(s, r, c, scale == 1.0);
    }
    for (long long i = 0; i < n_random - n_random / 2; ++i) {
        const double hb = std::ldexp(1.0 + rng.unit(), (int)(rng.unit() * 121.0) - 60) * (rng.unit() < 0.5 ? -1.0 : 1.0);
        const double disc = std::ldexp(1.0 + rng.unit(), (int)(rng.unit() * 241.0) - 120);
        const double a = std::ldexp(1.0 + rng.unit(), (int)(rng.unit() * 141.0) - 70);
        contain(hb, disc, a, c);
    }
    // ---- containment: constructed -------------------------------------------------------------
    const double tiny[] = {0.0, 4.9406564584124654e-324, 1e-300, 0x1.0p-80, 0x1.0p-81, 0x1.0p+80, 0x1.0p+81, kInf, kNaN};
    const double hbs[] = {0.0, -0.0, 1.0, -1.0, 1e-300, 1000.0, -1000.0, 0x1.0p+40, 0x1.0p+41, kInf, -kInf, kNaN};
    const double as[] = {0.0, 1.0, 0x1.0p-60, 0x1.0p-61, 0x1.0p+60, 0x1.0p+61, 0x1.0p-900, 0x1.0p-901, 0x1.0p+900, 0x1.0p+901,
                         1e-320, kInf, kNaN};
    for (double disc : tiny)
        for (double hb : hbs)
            for (double a : as) {
                contain(hb, disc, a, c);
                contain(hb, 1.0 + disc, a, c);
            }
    {   // infinite and NaN direction components, through a ray
        Sphere s{{0.0, 0.0, -1.0}, {0.0, 0.0, 0.0}, 0.5};
        const double bad[] = {kInf, -kInf, kNaN, 1e200, 1e-200};
        for (double x : bad)
            for (int a = 0; a < 3; ++a) {
                Ray r{};
                r.d[2] = -1.0;
                r.d[a] = x;
                contain_ray(s, r, c);
            }
    }

    // ---- equivalence --------------------------------------------------------------------------
    Equiv e;
    rtrb::Tally tally_scene, tally_rest;
    {   // scene 0's spheres, as lowered for the device (a Sphere is a MovingSphere of velocity 0)
        rtw::World w(1);
        if (rtw::build_scene(w, 0, nullptr, 0, 0)) return 1;
        std::string err;
        if (rtw::flatten(w, RT_ACCEL_SAH, err)) return 1;
        rtl::Lowered L;
        if (rtl::lower(w.flat.soa, true, L, err)) return 1;
        std::vector<Sphere> world;
        for (const rt_prim& p : L.leaf_prims) {
            if (p.kind > RT_PRIM_MOVING_SPHERE) return 1;
            world.push_back(Sphere{{p.p[0], p.p[1], p.p[2]}, {p.p[5], p.p[6], p.p[7]}, p.p[3]});
        }
        for (int i = 0; i < n_rays; ++i) compare(world, bounce_ray(world[(size_t)(rng.unit() * (double)world.size())], rng), rng, e, tally_scene);
    }
    {   // two identical spheres (the later-tested one wins), and centres 1 ulp, 1e-12 and 1e-7 apart
        const double gaps[] = {0.0, -1.0, 1e-12, 1e-7};
        for (double gap : gaps) {
            std::vector<Sphere> world;
            const double z0 = -3.0, z1 = gap < 0.0 ? std::nextafter(z0, 0.0) : z0 + gap;
            world.push_back(Sphere{{0.0, 0.0, z0}, {0.0, 0.0, 0.0}, 1.0});
            world.push_back(Sphere{{0.0, 0.0, z1}, {0.0, 0.0, 0.0}, 1.0});
            world.push_back(Sphere{{0.3, 0.2, z0}, {0.0, 0.0, 0.0}, 1.0});
            world.push_back(Sphere{{0.3, 0.2, z1}, {0.0, 0.0, 0.0}, 1.0});
            world.push_back(Sphere{{0.0, -1001.0, z0}, {0.0, 0.0, 0.0}, 1000.0});
            for (int i = 0; i < 400; ++i) {
                Ray r{};
                for (int a = 0; a < 3; ++a) r.o[a] = 0.2 * rng.sym();
                r.d[0] = 0.5 * rng.sym();
                r.d[1] = 0.5 * rng.sym();
                r.d[2] = -1.0 - rng.unit();
                compare(world, r, rng, e, tally_rest);
                compare(world, bounce_ray(world[(size_t)(i % 5)], rng), rng, e, tally_rest);   // from the surfaces too
            }
        }
    }
    {   // rays that meet NaN (sphere_t lets a NaN discriminant through and accepts the NaN root)
        std::vector<Sphere> world;
        world.push_back(Sphere{{0.0, 0.0, -3.0}, {0.0, 0.0, 0.0}, 1.0});
        world.push_back(Sphere{{0.0, 0.0, -6.0}, {0.0, 0.0, 0.0}, 1.0});
        world.push_back(Sphere{{0.0, kNaN, -4.0}, {0.0, 0.0, 0.0}, 0.5});
        world.push_back(Sphere{{0.0, 0.0, -2.0}, {0.0, 0.0, 0.0}, 0.25});
        for (int i = 0; i < 200; ++i) {
            Ray r{};
            r.d[0] = 0.1 * rng.sym();
            r.d[1] = 0.1 * rng.sym();
            r.d[2] = -1.0;
            compare(world, r, rng, e, tally_rest);
            Ray q = r;
            q.d[i % 3] = (i & 4) ? kNaN : kInf;
            compare(world, q, rng, e, tally_rest);
            Ray z = r;   // a zero direction: |d|^2 = 0, outside div_rcp's guard
            z.d[0] = z.d[1] = z.d[2] = 0.0;
            z.o[2] = -3.0;
            compare(world, z, rng, e, tally_rest);
        }
        world.pop_back();
        world.pop_back();   // without the NaN sphere: the plain rays again
        for (int i = 0; i < 50; ++i) {
            Ray r{};
            r.d[0] = 0.1 * rng.sym();
            r.d[1] = 0.1 * rng.sym();
            r.d[2] = -1.0;
            compare(world, r, rng, e, tally_rest);
        }
    }

    const long long scene_tests = tally_scene.bracket + tally_scene.exact;
    std::printf("{\"inputs\": %lld, \"valid\": %lld, \"ambiguous\": %lld, \"violations\": %lld, \"plain\": %lld, "
                "\"plain_valid\": %lld, \"worst\": %.4f, "
                "\"rays\": %lld, \"casts\": %lld, \"hits\": %lld, \"mismatches\": %lld, "
                "\"scene_tests\": %lld, \"scene_exact\": %lld, \"other_tests\": %lld, \"other_exact\": %lld}\n",
                c.inputs, c.valid, c.ambiguous, c.violations, c.plain, c.plain_valid, c.worst, e.rays, e.casts, e.hits,
                e.mismatches, scene_tests, tally_scene.exact, tally_rest.bracket + tally_rest.exact, tally_rest.exact);
    return c.violations == 0 && e.mismatches == 0 ? 0 : 1;
}
