// trace_prims.hpp — the megakernel's primitive tests (second layer of trace_device.hpp): spheres,
// rects and boxes as a t-only test for traversal and a finisher run once per cast, the f32 / f64
// slab tests of a node box, and simple_t / simple_finish over the primitive kinds.
#pragma once
#include "trace_types.hpp"

namespace rtk {

// ---------------------------------------------------------------------------
// primitives: a t-only test (traversal) and a finisher (once per cast)
// ---------------------------------------------------------------------------

// hittable.rs:254-273: the root in [t_min, t_max]
template <bool SMALL = false>
__device__ __forceinline__ bool sphere_t(double cx, double cy, double cz, double radius, const RayT<double>& r,
                                         double t_min, double t_max, double& t)
{
    const double ocx = r.ox - cx, ocy = r.oy - cy, ocz = r.oz - cz;
    const double half_b = ocx * r.dx + ocy * r.dy + ocz * r.dz;
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - radius * radius;
    const double disc = half_b * half_b - r.a * c;
    if (disc < 0.0) return false;
    const double sqrtd = __builtin_sqrt(disc);
    double root = div_rcp(-half_b - sqrtd, r.a, r.ya);
    if (root < t_min || t_max < root) {
        root = div_rcp(-half_b + sqrtd, r.a, r.ya);
        if (root < t_min || t_max < root) return false;
    }
    t = root;
    return true;
}

// sphere_t in two parts (CfgDefer, root_bracket.hpp): the quadratic's half_b and discriminant, in
// sphere_t's own expressions, and the root in [t_min, +inf) from them — the root sphere_t accepts
// a sphere with whatever its t_max (the near root if that is >= t_min, else the far one).
__device__ __forceinline__ void sphere_quad(double cx, double cy, double cz, double radius, const RayT<double>& r,
                                            double& half_b, double& disc)
{
    const double ocx = r.ox - cx, ocy = r.oy - cy, ocz = r.oz - cz;
    half_b = ocx * r.dx + ocy * r.dy + ocz * r.dz;
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - radius * radius;
    disc = half_b * half_b - r.a * c;
}
__device__ __forceinline__ bool sphere_root(double half_b, double disc, const RayT<double>& r, double t_min, double& t)
{
    const double sqrtd = __builtin_sqrt(disc);
    double root = div_rcp(-half_b - sqrtd, r.a, r.ya);
    if (root < t_min) {
        root = div_rcp(-half_b + sqrtd, r.a, r.ya);
        if (root < t_min) return false;
    }
    t = root;
    return true;
}

// A sphere-bounded ConstantMedium's two boundary queries (hittable.rs:430-434: hit over
// (-inf, inf), then over (t1 + 0.0001, inf)) from one quadratic: both calls of sphere_t above
// compute the same discriminant and roots, and differ only in the range the roots are checked
// against, so the pair (t1, t2) is theirs bit for bit; the second discriminant, sqrt and
// division are not computed again (round 5, VERDICT r04 item 6: the final scene's r = 5000
// fog sphere is queried by nearly every cast).
__device__ __forceinline__ bool sphere_t2(double cx, double cy, double cz, double radius, const RayT<double>& r,
                                          double& t1, double& t2)
{
    const double ocx = r.ox - cx, ocy = r.oy - cy, ocz = r.oz - cz;
    const double half_b = ocx * r.dx + ocy * r.dy + ocz * r.dz;
    const double c = (ocx * ocx + ocy * ocy + ocz * ocz) - radius * radius;
    const double disc = half_b * half_b - r.a * c;
    if (disc < 0.0) return false;   // both queries miss
    const double sqrtd = __builtin_sqrt(disc);
    const double near = div_rcp(-half_b - sqrtd, r.a, r.ya);
    // first query, (-inf, inf): the near root (no double lies outside it; a NaN root passes
    // sphere_t's range test too)
    t1 = near;
    const double lo = t1 + 0.0001;
    if (near < lo || RT_INF < near) {
        const double far = div_rcp(-half_b + sqrtd, r.a, r.ya);
        if (far < lo || RT_INF < far) return false;
        t2 = far;
    } else {
        t2 = near;
    }
    return true;
}

// f32 mode: c = |oc|^2 - r^2 and b/2 = oc . d of a sphere test. c of a large sphere is taken in
// f64 (an f32 c loses everything to cancellation on the r = 1000 ground sphere, whose surface
// every bounce starts on: |oc|^2 ~ 1e6, one f32 ulp 0.06); a small one's in f32, where the
// cancellation costs at most ~r^2 2^-24 (3e-6 at r <= 8), far below the t_min = 0.001 it must
// stay under. The random scene's BVH holds only r <= 1 spheres (its ground is the pre-leaf).
// SMALL: the spheres variant only (in the final-scene variant the second path costs spills;
// there it was no faster either: C4 1920x1080x100 f32 89.82 ms against 89.50 without; with the
// fast division 87.89 against 86.36; profiles/r06t_ab_f32final_c4.log).
#ifndef RT_F32_SMALL_SPHERE
#define RT_F32_SMALL_SPHERE 8.0
#endif
template <bool SMALL = false>
__device__ __forceinline__ void sphere_cb(double cx, double cy, double cz, double radius, const RayT<float>& r,
                                          float& c, float& half_b)
{
    if (SMALL && radius <= RT_F32_SMALL_SPHERE) {
        const float ox = r.ox - (float)cx, oy = r.oy - (float)cy, oz = r.oz - (float)cz;
        const float rf = (float)radius;
        c = (ox * ox + oy * oy + oz * oz) - rf * rf;
        half_b = ox * r.dx + oy * r.dy + oz * r.dz;
        return;
    }
    const double ocx = (double)r.ox - cx, ocy = (double)r.oy - cy, ocz = (double)r.oz - cz;
    c = (float)((ocx * ocx + ocy * ocy + ocz * ocz) - radius * radius);
    half_b = (float)ocx * r.dx + (float)ocy * r.dy + (float)ocz * r.dz;
}

// f32 mode: sphere_t's f32 roots, the same selection (its second query starts at
// t1 + max(1e-4, |t1| 2^-19), medium_t)
__device__ __forceinline__ bool sphere_t2(double cx, double cy, double cz, double radius, const RayT<float>& r,
                                          float& t1, float& t2)
{
    float c, half_b;
    sphere_cb(cx, cy, cz, radius, r, c, half_b);
    const float disc = half_b * half_b - r.a * c;
    if (disc < 0.0f) return false;
    const float q = -(half_b + __builtin_copysignf(__builtin_sqrtf(disc), half_b));
    const float r0 = c / q, r1 = q / r.a;
    const float tn = fminf(r0, r1), tf = fmaxf(r0, r1);
    t1 = tn;
    const float lo = t1 + fmaxf(0.0001f, __builtin_fabsf(t1) * 0x1.0p-19f);
    float root = tn;
    if (root < lo || (float)RT_INF < root) {
        root = tf;
        if (root < lo || (float)RT_INF < root) return false;
    }
    t2 = root;
    return true;
}

// f32 mode: the same roots, robust in f32 (Haines et al., Ray Tracing Gems ch. 7): c as
// sphere_cb takes it, the near root as c / q (Vieta) instead of the cancelling -b - sqrt(disc).
template <bool SMALL = false>
__device__ __forceinline__ bool sphere_t(double cx, double cy, double cz, double radius, const RayT<float>& r,
                                         float t_min, float t_max, float& t)
{
    float c, half_b;
    sphere_cb<SMALL>(cx, cy, cz, radius, r, c, half_b);
    const float disc = half_b * half_b - r.a * c;
    if (disc < 0.0f) return false;
    const float q = -(half_b + __builtin_copysignf(__builtin_sqrtf(disc), half_b));
    const float t0 = c / q, t1 = q / r.a;
    const float tn = fminf(t0, t1), tf = fmaxf(t0, t1);
    float root = tn;
    if (root < t_min || t_max < root) {
        root = tf;
        if (root < t_min || t_max < root) return false;
    }
    t = root;
    return true;
}

// Whether hit records carry the texture coordinates' inputs (uv0..uv3). Without FEAT_IMAGE_UV
// the only image-textured primitives are top-level spheres, whose outward normal — the
// sphere_uv input — is the record's normal, negated back when the hit was on the back face
// (exact): the final scene's records then keep 8 VGPRs fewer live across the bounce loop.
template <class C>
constexpr bool UVStore()
{
    return (C::F & FEAT_IMAGE) != 0 && (C::F & FEAT_IMAGE_UV) != 0;
}

// hittable.rs:275-287
template <class C, class R = typename C::Real>
__device__ __forceinline__ void sphere_finish(R cx, R cy, R cz, R inv_r, const RayT<R>& r, R t, int mat, HitT<R>& h)
{
    h.t = t;
    h.px = r.ox + r.dx * t;
    h.py = r.oy + r.dy * t;
    h.pz = r.oz + r.dz * t;
    const R onx = (h.px - cx) * inv_r, ony = (h.py - cy) * inv_r, onz = (h.pz - cz) * inv_r;
    set_face_normal(h, r.dx, r.dy, r.dz, onx, ony, onz);
    h.mat = mat;
    h.uvkind = 1;
    if constexpr (UVStore<C>()) {
        h.uv0 = onx;
        h.uv1 = ony;
        h.uv2 = onz;
    }
}

// hittable.rs:308-320 (axis 0: XY, k on z; 1: XZ, k on y; 2: YZ, k on x)
template <class R>
__device__ __forceinline__ void rect_axes(int axis, const RayT<R>& r, R& ok, R& dk, R& oa, R& da, R& ob, R& db)
{
    if (axis == 0) { ok = r.oz; dk = r.dz; oa = r.ox; da = r.dx; ob = r.oy; db = r.dy; }
    else if (axis == 1) { ok = r.oy; dk = r.dy; oa = r.ox; da = r.dx; ob = r.oz; db = r.dz; }
    else { ok = r.ox; dk = r.dx; oa = r.oy; da = r.dy; ob = r.oz; db = r.dz; }
}

template <bool RCP = false, class R>
__device__ __forceinline__ bool rect_t(int axis, R a0, R a1, R b0, R b1, R k, const RayT<R>& r, R t_min, R t_max,
                                       R& t_out)
{
    R ok, dk, oa, da, ob, db;
    rect_axes(axis, r, ok, dk, oa, da, ob, db);
    R t;
    if constexpr (RCP) {
        // (k - o) / d through the ray's correctly rounded 1/d: the same bits (div_rcp), 3 FMAs
        // instead of a division per rect (a Box tests 6)
        const R yk = axis == 0 ? r.yz : axis == 1 ? r.yy : r.yx;
        t = div_rcp(k - ok, dk, yk);
    } else {
        t = (k - ok) / dk;
    }
    if (t < t_min || t > t_max) return false;
    const R x = oa + t * da;
    const R y = ob + t * db;
    if (x < a0 || x > a1 || y < b0 || y > b1) return false;
    t_out = t;
    return true;
}

// rect_t with the caller's RN(1 / d_axis), |d_axis| in [2^-900, 2^900] (div_rcp: the division's bits)
__device__ __forceinline__ bool rect_t_y(int axis, double a0, double a1, double b0, double b1, double k,
                                         const RayT<double>& r, double yk, double t_min, double t_max, double& t_out)
{
    double ok, dk, oa, da, ob, db;
    rect_axes(axis, r, ok, dk, oa, da, ob, db);
    const double q = k - ok, q0 = q * yk;   // div_rcp without its guard (the caller checked the range)
    const double t = __builtin_fma(__builtin_fma(-dk, q0, q), yk, q0);
    if (t < t_min || t > t_max) return false;
    const double x = oa + t * da;
    const double y = ob + t * db;
    if (x < a0 || x > a1 || y < b0 || y > b1) return false;
    t_out = t;
    return true;
}
template <class R>
__device__ __forceinline__ bool rect_t_y(int, R, R, R, R, R, const RayT<R>&, R, R, R, R&) { return false; }

// hittable.rs:322-331
template <class C, class R = typename C::Real>
__device__ __forceinline__ void rect_finish(int axis, R a0, R a1, R b0, R b1, const RayT<R>& r, R t, int mat,
                                            HitT<R>& h)
{
    R ok, dk, oa, da, ob, db;
    rect_axes(axis, r, ok, dk, oa, da, ob, db);
    h.uvkind = 2;
    if constexpr (UVStore<C>()) {
        const R x = oa + t * da;
        const R y = ob + t * db;
        h.uv0 = x - a0;
        h.uv1 = a1 - a0;
        h.uv2 = y - b0;
        h.uv3 = b1 - b0;
    }
    h.t = t;
    set_face_normal(h, r.dx, r.dy, r.dz, axis == 2 ? (R)1 : (R)0, axis == 1 ? (R)1 : (R)0, axis == 0 ? (R)1 : (R)0);
    h.mat = mat;
    h.px = r.ox + r.dx * t;
    h.py = r.oy + r.dy * t;
    h.pz = r.oz + r.dz * t;
}

// slab tests of an f32 box (BVH nodes, Box pre-tests)
template <class RayType>
__device__ __forceinline__ bool slab32(const float* lo, const float* hi, const RayType& r, float t_min, float t_max,
                                       float& t_near)
{
    const float x0 = __builtin_fmaf(lo[0], r.sx.x, r.sx.y), x1 = __builtin_fmaf(hi[0], r.sx.x, r.sx.y);
    const float y0 = __builtin_fmaf(lo[1], r.sy.x, r.sy.y), y1 = __builtin_fmaf(hi[1], r.sy.x, r.sy.y);
    const float z0 = __builtin_fmaf(lo[2], r.sz.x, r.sz.y), z1 = __builtin_fmaf(hi[2], r.sz.x, r.sz.y);
    const float tn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), t_min));
    const float tf = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), t_max));
    t_near = tn;
    return tn <= tf;
}

// f32 bounds of a double t range, rounded outward
template <class R>
__device__ __forceinline__ float f32_down(R t)
{
    const float f = (float)t;
    return f > 0.0f ? f * (1.0f - 0x1.0p-20f) : f * (1.0f + 0x1.0p-20f);
}
template <class R>
__device__ __forceinline__ float f32_up(R t)
{
    const float f = (float)t;
    return f > 0.0f ? f * (1.0f + 0x1.0p-20f) : f * (1.0f - 0x1.0p-20f);
}

// Conservative slab test against an f32 box (rounded outward and padded on the
// host), in f64. NaN products (0 * inf) are ignored by fmin/fmax.
template <class R>
__device__ __forceinline__ bool slab(const float* lo, const float* hi, const RayT<R>& r, R t_min, R t_max, R& t_near)
{
    const R x0 = ((R)lo[0] - r.ox) * r.ix, x1 = ((R)hi[0] - r.ox) * r.ix;
    const R y0 = ((R)lo[1] - r.oy) * r.iy, y1 = ((R)hi[1] - r.oy) * r.iy;
    const R z0 = ((R)lo[2] - r.oz) * r.iz, z1 = ((R)hi[2] - r.oz) * r.iz;
    const R tn = fmax(fmax(fmin(x0, x1), fmin(y0, y1)), fmax(fmin(z0, z1), t_min));
    const R tf = fmin(fmin(fmax(x0, x1), fmax(y0, y1)), fmin(fmax(z0, z1), t_max));
    t_near = tn;
    return tn <= tf;
}

// the six sides of new_box (hittable.rs:135-142): side -> axis, (a0 a1 b0 b1 k) from min/max
template <class R>
__device__ __forceinline__ void box_side(const rt_prim& p, int side, int& axis, R& a0, R& a1, R& b0, R& b1, R& k)
{
    const R mnx = (R)p.p[0], mny = (R)p.p[1], mnz = (R)p.p[2], mxx = (R)p.p[3], mxy = (R)p.p[4], mxz = (R)p.p[5];
    if (side < 2) { axis = 0; a0 = mnx; a1 = mxx; b0 = mny; b1 = mxy; k = side == 0 ? mxz : mnz; }
    else if (side < 4) { axis = 1; a0 = mnx; a1 = mxx; b0 = mnz; b1 = mxz; k = side == 2 ? mxy : mny; }
    else { axis = 2; a0 = mny; a1 = mxy; b0 = mnz; b1 = mxz; k = side == 4 ? mxx : mnx; }
}

// Box::hit = hit_hittables over its sides (hittable.rs:229-231): closest, ties to the later side.
// No bounding-box pre-test, like the reference (Q8): a per-box slab pre-test and per-side
// candidate tests both measured slower (a lane that skips a test saves the wave nothing unless
// every lane does).
template <bool RCP = false, bool LRCP = false, class R>
__device__ __forceinline__ bool box_t(const rt_prim& p, const RayT<R>& r, R t_min, R t_max, R& t, int& side)
{
    bool any = false;
    // f64: the six sides divide by three directions; one correctly rounded reciprocal y per
    // direction and a Markstein step per side (RN(q / d) bit for bit when y = RN(1 / d): see
    // div_rcp) instead of six divisions. The range guard is taken once per box (a ray with a
    // direction component outside [2^-900, 2^900], e.g. an exact 0, divides as the reference).
    constexpr bool LOCAL_RCP = LRCP && !RCP && std::is_same<R, double>::value;
    auto in_range = [](R d) { const R m = r_fabs(d); return m >= (R)0x1.0p-900 && m <= (R)0x1.0p+900; };
    if (LOCAL_RCP && in_range(r.dx) && in_range(r.dy) && in_range(r.dz)) {
        R y = (R)0;   // of the side pair's direction (sides 2a, 2a+1 share axis a)
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            int axis;
            R a0, a1, b0, b1, k, ts;
            box_side(p, s, axis, a0, a1, b0, b1, k);
            if ((s & 1) == 0) y = (R)1 / (s == 0 ? r.dz : s == 2 ? r.dy : r.dx);
            if (rect_t_y(axis, a0, a1, b0, b1, k, r, y, t_min, t_max, ts)) {
                t_max = ts;
                t = ts;
                side = s;
                any = true;
            }
        }
        return any;
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        int axis;
        R a0, a1, b0, b1, k, ts;
        box_side(p, s, axis, a0, a1, b0, b1, k);
        if (rect_t<RCP>(axis, a0, a1, b0, b1, k, r, t_min, t_max, ts)) {
            t_max = ts;
            t = ts;
            side = s;
            any = true;
        }
    }
    return any;
}

// The centre of a Sphere, or of a MovingSphere at the ray's time: center_0 +
// ((time - time_0) / (time_1 - time_0)) * (center_1 - center_0) (hittable.rs:556-558).
// Both kinds go through one code path with no select: the upload stores a Sphere as a
// MovingSphere of velocity 0 (scene_lower.cpp), whose c0 + 0 * s is c0 bit for bit (s finite), so
// a wave whose lanes hold both kinds runs one test and loads no kind.
template <class R>
__device__ __forceinline__ void sphere_center(const rt_prim& p, const RayT<R>& r, bool general, double& cx, double& cy,
                                              double& cz, bool is_static = false)
{
    if (is_static) {   // FEAT_STATIC: a Sphere, whose c0 + 0 * s is c0 bit for bit
        cx = p.p[0];
        cy = p.p[1];
        cz = p.p[2];
        return;
    }
    double s = (double)r.time;
    // general: the variant has FEAT_SHUTTER (no reference scene does: their moving spheres
    // all have the [0, 1] shutter); without it the flag is not loaded at all
    if (general && !p.a) s = ((double)r.time - p.p[8]) / (p.p[9] - p.p[8]);   // a MovingSphere with a general shutter
    cx = p.p[0] + p.p[5] * s;
    cy = p.p[1] + p.p[6] * s;
    cz = p.p[2] + p.p[7] * s;
}

// Sphere, MovingSphere, rects, Box: t-only (hittable.rs:211-231).
template <class C, class R = typename C::Real>
__device__ __forceinline__ bool simple_t(const rt_prim& p, const RayT<R>& r, R t_min, R t_max, R& t, int& side,
                                         Count& cnt, bool gs)
{
    if (C::COUNT) cnt.prims++;
    if (!(C::F & FEAT_RECT) || p.kind <= RT_PRIM_MOVING_SPHERE) {
        double cx, cy, cz;
        sphere_center(p, r, gs, cx, cy, cz, (C::F & FEAT_STATIC) != 0);
        return sphere_t<C::F == FEAT_SET_SPHERES>(cx, cy, cz, p.p[3], r, t_min, t_max, t);
    } else {
        const R q0 = (R)p.p[0], q1 = (R)p.p[1], q2 = (R)p.p[2], q3 = (R)p.p[3], q4 = (R)p.p[4];
        switch (p.kind) {
        case RT_PRIM_XY_RECT: return rect_t<RectRcp<C>()>(0, q0, q1, q2, q3, q4, r, t_min, t_max, t);
        case RT_PRIM_XZ_RECT: return rect_t<RectRcp<C>()>(1, q0, q1, q2, q3, q4, r, t_min, t_max, t);
        case RT_PRIM_YZ_RECT: return rect_t<RectRcp<C>()>(2, q0, q1, q2, q3, q4, r, t_min, t_max, t);
        case RT_PRIM_BOX: return box_t<RectRcp<C>(), BoxRcp<C>()>(p, r, t_min, t_max, t, side);
        default: return false;
        }
    }
}

template <class C, class R = typename C::Real>
__device__ __forceinline__ void simple_finish(const rt_prim& p, const RayT<R>& r, R t, int side, HitT<R>& h, bool gs)
{
    if constexpr ((C::F & FEAT_RECT) != 0) {
        if (p.kind >= RT_PRIM_XY_RECT && p.kind <= RT_PRIM_YZ_RECT) {
            rect_finish<C>(p.kind - RT_PRIM_XY_RECT, (R)p.p[0], (R)p.p[1], (R)p.p[2], (R)p.p[3], r, t, p.mat, h);
            return;
        }
        if (p.kind == RT_PRIM_BOX) {
            int axis;
            R a0, a1, b0, b1, k;
            box_side(p, side, axis, a0, a1, b0, b1, k);
            rect_finish<C>(axis, a0, a1, b0, b1, r, t, p.mat, h);
            return;
        }
    }
    double cx, cy, cz;
    sphere_center(p, r, gs, cx, cy, cz, (C::F & FEAT_STATIC) != 0);
    sphere_finish<C>((R)cx, (R)cy, (R)cz, (R)p.p[4], r, t, p.mat, h);
}

}  // namespace rtk
