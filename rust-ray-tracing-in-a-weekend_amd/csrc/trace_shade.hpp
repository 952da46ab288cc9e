// trace_shade.hpp — the megakernel's shading layer (fourth layer of trace_device.hpp): Perlin noise
// and textures, the path's random stream and draws, the camera, the material / texture tables and
// the block prologue that stages them with the BVH nodes in LDS (stage_lds), and one hit of
// ray_color in its three steps (shade_begin, the draws, shade_end).
#pragma once
#include "trace_walk.hpp"

namespace rtk {

// ---------------------------------------------------------------------------
// appearance: texture.rs:30-75, perlin.rs:32-108, material.rs:15-94
// ---------------------------------------------------------------------------
template <class R>
__device__ R perlin_noise(const double* ranvec, const int32_t* perm, R px, R py, R pz)
{
    const R fx = r_floor(px), fy = r_floor(py), fz = r_floor(pz);
    R u = px - fx, v = py - fy, w = pz - fz;
    u = u * u * ((R)3 - (R)2 * u);
    v = v * v * ((R)3 - (R)2 * v);
    w = w * w * ((R)3 - (R)2 * w);
    const int32_t i = r_sat_i32(fx), j = r_sat_i32(fy), k = r_sat_i32(fz);
    const R uu = u * u * ((R)3 - (R)2 * u);
    const R vv = v * v * ((R)3 - (R)2 * v);
    const R ww = w * w * ((R)3 - (R)2 * w);
    R accum = (R)0;
    // (the corner and octave loops unrolled: rolled measured slower, C4 143.3 vs 136.9 ms,
    // r03b_ab_c4.log)
#pragma unroll
    for (int di = 0; di < 2; ++di)
#pragma unroll
        for (int dj = 0; dj < 2; ++dj)
#pragma unroll
            for (int dk = 0; dk < 2; ++dk) {
                const uint32_t xi = ((uint32_t)i + (uint32_t)di) & 255u;
                const uint32_t yi = ((uint32_t)j + (uint32_t)dj) & 255u;
                const uint32_t zi = ((uint32_t)k + (uint32_t)dk) & 255u;
                const uint32_t idx = (uint32_t)(perm[xi] ^ perm[256 + yi] ^ perm[512 + zi]) & 255u;
                const R cx = (R)ranvec[3 * idx], cy = (R)ranvec[3 * idx + 1], cz = (R)ranvec[3 * idx + 2];
                const R fi = (R)di, fj = (R)dj, fk = (R)dk;
                const R wx = u - fi, wy = v - fj, wz = w - fk;
                accum += (fi * uu + ((R)1 - fi) * ((R)1 - uu)) * (fj * vv + ((R)1 - fj) * ((R)1 - vv)) *
                         (fk * ww + ((R)1 - fk) * ((R)1 - ww)) * (cx * wx + cy * wy + cz * wz);
            }
    return accum;
}

template <class R>
__device__ R perlin_turb(const double* ranvec, const int32_t* perm, R px, R py, R pz)
{
    R accum = (R)0, weight = (R)1;
    for (int i = 0; i < 7; ++i) {
        accum += weight * perlin_noise(ranvec, perm, px, py, pz);
        weight *= (R)0.5;
        px = px * (R)2;
        py = py * (R)2;
        pz = pz * (R)2;
    }
    return r_fabs(accum);
}

template <class R>
__device__ __forceinline__ R clampd(R x, R mn, R mx)
{
    if (x < mn) return mn;
    if (x > mx) return mx;
    return x;
}

template <class C, class R>
__device__ void hit_uv(const HitT<R>& h, R& u, R& v)
{
    if (h.uvkind == 1) {  // sphere_uv (math.rs:288-300)
        R ox = h.uv0, oy = h.uv1, oz = h.uv2;
        if constexpr (!UVStore<C>()) {   // the outward normal (set_face_normal negated it on a back face)
            ox = h.front ? h.nx : -h.nx;
            oy = h.front ? h.ny : -h.ny;
            oz = h.front ? h.nz : -h.nz;
        }
        const R theta = r_acos(-oy);
        const R phi = r_atan2(-oz, ox) + (R)RT_PI;
        u = phi / ((R)2 * (R)RT_PI);
        v = theta / (R)RT_PI;
    } else if (h.uvkind == 2) {
        u = h.uv0 / h.uv1;
        v = h.uv2 / h.uv3;
    } else {
        u = (R)0;
        v = (R)0;
    }
}

// texture.rs:35-41: sin(10x)*sin(10y)*sin(10z) < 0 from the three signs (rt_sin_sign);
// the full product only when a factor may be tiny enough to underflow it
// f32 mode: the same sign test without the three sinf: sin(10a) < 0 exactly when floor(10a / pi)
// is odd, so the product is negative when the three floors sum to an odd number (the zeros of a
// factor, where the reference's product is 0 and not < 0, are a measure-zero set)
__device__ __forceinline__ bool checker_odd(const HitT<float>& h)
{
    constexpr float k = (float)(10.0 / 3.14159265358979323846);
    const int n = (int)__builtin_floorf(h.px * k) + (int)__builtin_floorf(h.py * k) + (int)__builtin_floorf(h.pz * k);
    return (n & 1) != 0;
}
__device__ __forceinline__ bool checker_odd(const HitT<double>& h)
{
    const double ax = 10.0 * h.px, ay = 10.0 * h.py, az = 10.0 * h.pz;
    const int sx = rt_sin_sign(ax), sy = rt_sin_sign(ay), sz = rt_sin_sign(az);
    if (sx == 2 || sy == 2 || sz == 2) return rt_sin(ax) * rt_sin(ay) * rt_sin(az) < 0.0;
    return sx * sy * sz < 0;
}

template <class C>
__device__ __forceinline__ const rt_texture& texture_of(const SceneDev& S, int i);

template <class C, class R = typename C::Real>
__device__ void tex_value(const SceneDev& S, int ti, const HitT<R>& h, R& cr, R& cg, R& cb)
{
    const rt_texture& t = texture_of<C>(S, ti);
    if constexpr (!(C::F & (FEAT_NOISE | FEAT_IMAGE))) {
        if (t.kind == RT_TEX_CHECKER) {
            const double* c = checker_odd(h) ? t.c1 : t.c0;
            cr = (R)c[0]; cg = (R)c[1]; cb = (R)c[2];
        } else {
            cr = (R)t.c0[0]; cg = (R)t.c0[1]; cb = (R)t.c0[2];
        }
        return;
    }
    switch (t.kind) {
    case RT_TEX_SOLID: cr = (R)t.c0[0]; cg = (R)t.c0[1]; cb = (R)t.c0[2]; return;
    case RT_TEX_CHECKER: {
        if (checker_odd(h)) { cr = (R)t.c1[0]; cg = (R)t.c1[1]; cb = (R)t.c1[2]; }
        else { cr = (R)t.c0[0]; cg = (R)t.c0[1]; cb = (R)t.c0[2]; }
        return;
    }
    case RT_TEX_NOISE: {
        const double* rv = S.perlin_ranvec + (size_t)t.perlin * 768;
        const int32_t* pm = S.perlin_perm + (size_t)t.perlin * 768;
        const R s = (R)1 + r_sin((R)t.scale * h.pz + (R)10 * perlin_turb(rv, pm, h.px, h.py, h.pz));
        const R c = (R)1 * (R)0.5 * s;
        cr = c; cg = c; cb = c;
        return;
    }
    default: {
        if (t.img_w <= 0 || t.img_h <= 0) { cr = (R)0; cg = (R)1; cb = (R)1; return; }
        R u, v;
        hit_uv<C>(h, u, v);
        u = clampd(u, (R)0, (R)1);
        v = (R)1 - clampd(v, (R)0, (R)1);
        uint64_t i = r_sat_u64(u * (R)t.img_w);
        uint64_t j = r_sat_u64(v * (R)t.img_h);
        if (i >= (uint64_t)t.img_w) i = (uint64_t)t.img_w - 1;
        if (j >= (uint64_t)t.img_h) j = (uint64_t)t.img_h - 1;
        const uint8_t* px = S.image + t.img_offset + j * (uint64_t)t.img_bps + i * 3;
        const R color_scale = (R)1 / (R)255;
        cr = color_scale * (R)px[0];
        cg = color_scale * (R)px[1];
        cb = color_scale * (R)px[2];
        return;
    }
    }
}

// The path stream of rt_numerics.h (rt_pstream): one Philox block of (pixel, sample) seeds
// a xoshiro128++ state, from which the path draws in the reference's order.
__device__ __forceinline__ void ds_start(rt_pstream& st, uint64_t seed, uint32_t pixel, uint32_t sample)
{
    rt_pstream_init(&st, seed, pixel, sample);
}
// The f32 mode's path stream: the same counter and key through 7 Philox rounds instead of 10
// (Salmon et al., SC'11: Philox4x32-7 already passes TestU01's BigCrush; the f64 mode keeps the
// 10 rounds of the protocol the oracle restates). 30 % fewer of the per-sample
// seeding's 32x32-bit products, which take ~7 % of the f32 kernel on the random scene.
#ifndef RT_F32_PHILOX_ROUNDS
#define RT_F32_PHILOX_ROUNDS 7
#endif
__device__ __forceinline__ void ds_start_f32(rt_pstream& st, uint64_t seed, uint32_t pixel, uint32_t sample)
{
    rt_u32x4 c;
    c.v[0] = pixel; c.v[1] = sample; c.v[2] = 0; c.v[3] = RT_STREAM_PATH;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < RT_F32_PHILOX_ROUNDS; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.v[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c.v[2];
        rt_u32x4 n;
        n.v[0] = (uint32_t)(p1 >> 32) ^ c.v[1] ^ k0;
        n.v[1] = (uint32_t)p1;
        n.v[2] = (uint32_t)(p0 >> 32) ^ c.v[3] ^ k1;
        n.v[3] = (uint32_t)p0;
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    st.s0 = c.v[0]; st.s1 = c.v[1]; st.s2 = c.v[2]; st.s3 = c.v[3];
    if ((st.s0 | st.s1 | st.s2 | st.s3) == 0) st.s0 = 1;
}
__device__ __forceinline__ uint64_t ds_u64(rt_pstream& st) { return rt_pstream_u64(&st); }

// The path's draws. f64: rand's Standard / gen_range mappings of 64-bit draws (math.rs:268-280,
// rt_numerics.h); f32 mode: one 32-bit draw each, 24 significant bits.
__device__ __forceinline__ double draw_unit(rt_pstream& st, double) { return rt_unit53(ds_u64(st)); }
__device__ __forceinline__ float draw_unit(rt_pstream& st, float)
{
    return (float)(rt_pstream_u32(&st) >> 8) * 0x1.0p-24f;
}
__device__ __forceinline__ double draw_m11(rt_pstream& st, double scale_m11) { return rt_uniform_sample(ds_u64(st), -1.0, scale_m11); }
__device__ __forceinline__ float draw_m11(rt_pstream& st, float)
{
    return (float)(rt_pstream_u32(&st) >> 8) * 0x1.0p-23f - 1.0f;
}

// math.rs:51-58: random_double_range(-1, 1) x 3 until inside
template <class R>
__device__ __forceinline__ void random_in_unit_sphere(rt_pstream& st, R scale_m11, R& x, R& y, R& z, R& len2)
{
    for (;;) {
        x = draw_m11(st, scale_m11);
        y = draw_m11(st, scale_m11);
        z = draw_m11(st, scale_m11);
        len2 = x * x + y * y + z * z;
        if (len2 < (R)1) return;
    }
}

// ---------------------------------------------------------------------------
// the integrator
// ---------------------------------------------------------------------------

// main.rs:517-520 + Camera::get_ray (camera.rs:58-66) in three steps: camera_begin (the
// pixel jitter draws), the lens draws (random_in_unit_disk: 2 draws per try, the same
// mapping as random_in_unit_sphere's, whose loop the pool schedules share with it) and
// camera_end (the ray and its time draw). camera_ray runs them in a row.
__device__ __forceinline__ void camera_begin(const KParams& P, int x, int y, rt_pstream& st, float& u, float& v)
{   // f32 mode
    u = ((float)x + draw_unit(st, 0.0f)) / (float)P.wm1;
    v = ((float)y + draw_unit(st, 0.0f)) / (float)P.hm1;
}
__device__ __forceinline__ void camera_begin(const KParams& P, int x, int y, rt_pstream& st, double& u, double& v)
{
    u = div_rcp((double)x + rt_unit53(ds_u64(st)), P.wm1, P.inv_wm1);
    v = div_rcp((double)y + rt_unit53(ds_u64(st)), P.hm1, P.inv_hm1);
}
// one try of random_in_unit_disk (3 = false) or random_in_unit_sphere (3 = true): the
// length test of a disk candidate is x*x + y*y + 0*0, the same value as x*x + y*y
template <class R>
__device__ __forceinline__ bool unit_try(rt_pstream& st, R scale_m11, bool three, R& x, R& y, R& z, R& len2)
{
    x = draw_m11(st, scale_m11);
    y = draw_m11(st, scale_m11);
    z = (R)0;
    if (three) z = draw_m11(st, scale_m11);
    len2 = x * x + y * y + z * z;
    return len2 < (R)1;
}
__device__ __forceinline__ void camera_end(const KParams& P, rt_pstream& st, float u, float v, float dxl, float dyl,
                                           RayT<float>& r)
{   // f32 mode
    const rt_camera& c = P.cam;
    const float rdx = dxl * (float)c.lens_radius, rdy = dyl * (float)c.lens_radius;
    const float offx = (float)c.u[0] * rdx + (float)c.v[0] * rdy;
    const float offy = (float)c.u[1] * rdx + (float)c.v[1] * rdy;
    const float offz = (float)c.u[2] * rdx + (float)c.v[2] * rdy;
    r.ox = (float)c.origin[0] + offx;
    r.oy = (float)c.origin[1] + offy;
    r.oz = (float)c.origin[2] + offz;
    // lower_left_corner - origin folded in f64 on the way (one rounding instead of two)
    r.dx = (float)(c.lower_left_corner[0] - c.origin[0]) + (float)c.horizontal[0] * u + (float)c.vertical[0] * v - offx;
    r.dy = (float)(c.lower_left_corner[1] - c.origin[1]) + (float)c.horizontal[1] * u + (float)c.vertical[1] * v - offy;
    r.dz = (float)(c.lower_left_corner[2] - c.origin[2]) + (float)c.horizontal[2] * u + (float)c.vertical[2] * v - offz;
    r.time = (float)c.time0 + draw_unit(st, 0.0f) * (float)(c.time1 - c.time0);
}
__device__ __forceinline__ void camera_end(const KParams& P, rt_pstream& st, double u, double v, double dxl,
                                           double dyl, RayT<double>& r)
{
    const double rdx = dxl * P.cam.lens_radius, rdy = dyl * P.cam.lens_radius;
    const double offx = P.cam.u[0] * rdx + P.cam.v[0] * rdy;
    const double offy = P.cam.u[1] * rdx + P.cam.v[1] * rdy;
    const double offz = P.cam.u[2] * rdx + P.cam.v[2] * rdy;
    r.ox = P.cam.origin[0] + offx;
    r.oy = P.cam.origin[1] + offy;
    r.oz = P.cam.origin[2] + offz;
    r.dx = P.cam.lower_left_corner[0] + P.cam.horizontal[0] * u + P.cam.vertical[0] * v - P.cam.origin[0] - offx;
    r.dy = P.cam.lower_left_corner[1] + P.cam.horizontal[1] * u + P.cam.vertical[1] * v - P.cam.origin[1] - offy;
    r.dz = P.cam.lower_left_corner[2] + P.cam.horizontal[2] * u + P.cam.vertical[2] * v - P.cam.origin[2] - offz;
    r.time = rt_uniform_sample(ds_u64(st), P.cam.time0, P.scale_time);
}
template <class R>
__device__ __forceinline__ void camera_ray(const KParams& P, int x, int y, rt_pstream& st, RayT<R>& r)
{
    R u, v, dxl, dyl, dzl, l2;
    camera_begin(P, x, y, st, u, v);
    while (!unit_try(st, (R)P.scale_m11, false, dxl, dyl, dzl, l2)) {
    }
    camera_end(P, st, u, v, dxl, dyl, r);
}

template <class C>
__device__ __forceinline__ int lds_stack_offset(const SceneDev& S)   // in ints, after the TLAS nodes
{
    return (int)(lds_layout_of<C>(S).stack / 4);
}
template <class C>
__device__ __forceinline__ int lds_shade_offset(const SceneDev& S)   // in ints
{
    return (int)(lds_layout_of<C>(S).shade / 4);
}
template <class C>
__device__ __forceinline__ const rt_material& material_of(const SceneDev& S, int i)
{
    if constexpr (StageShade<C>()) {
        if (S.n_lds_materials > 0)
            return reinterpret_cast<const rt_material*>(rt_lds + lds_shade_offset<C>(S))[i];
    }
    return S.materials[i];
}
template <class C>
__device__ __forceinline__ const rt_texture& texture_of(const SceneDev& S, int i)
{
    if constexpr (StageShade<C>()) {
        if (S.n_lds_materials > 0)
            return reinterpret_cast<const rt_texture*>(rt_lds + lds_shade_offset<C>(S) + S.n_lds_materials * 16)[i];
    }
    return S.textures[i];
}
// block prologue: TLAS nodes, then the material and texture tables (every thread takes part)
template <class C>
__device__ __forceinline__ void stage_lds(const SceneDev& S)
{
    bool any = false;
    const int off = 0;   // the TLAS nodes first (traverse)
    if (S.n_lds_nodes > 0) {
        if constexpr (OctNodes<C>()) {   // one node per thread, rt_bvh_node -> LdsNode
            LdsNode* dst = reinterpret_cast<LdsNode*>(rt_lds + off);
            for (int i = threadIdx.x; i < S.n_lds_nodes; i += BlockThreads<C>()) {
                const rt_bvh_node n = S.nodes[i];
                LdsNode o;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    o.ax[a][0] = n.lo0[a]; o.ax[a][1] = n.lo1[a];
                    o.ax[a][2] = n.hi0[a]; o.ax[a][3] = n.hi1[a];
                    o.ax[a][4] = n.lo0[a]; o.ax[a][5] = n.lo1[a];
                }
#pragma unroll
                for (int c = 0; c < 2; ++c)   // node references: LDS addresses (leaf codes stay < 0)
                    o.child[c] = n.child[c] >= 0 ? (int)(lds_addr(dst) + (uint32_t)n.child[c] * (uint32_t)sizeof(LdsNode))
                                                 : n.child[c];
                dst[i] = o;
            }
        } else {
            uint4* dst = reinterpret_cast<uint4*>(rt_lds + off);
            const uint4* src = reinterpret_cast<const uint4*>(S.nodes);
            for (int i = threadIdx.x; i < S.n_lds_nodes * 4; i += BlockThreads<C>()) dst[i] = src[i];
        }
        any = true;
    }
    if constexpr (StageBlas<C>()) {
        if (S.n_lds_blas > 0) {   // the BLAS's BFS prefix, nodes[n_tlas_nodes, ...) (scene_lower.cpp)
            uint4* db = reinterpret_cast<uint4*>(reinterpret_cast<char*>(rt_lds) + lds_layout_of<C>(S).blas);
            const uint4* sb = reinterpret_cast<const uint4*>(S.nodes + S.n_tlas_nodes);
            for (int i = threadIdx.x; i < S.n_lds_blas * 4; i += BlockThreads<C>()) db[i] = sb[i];
            any = true;
        }
    }
    if constexpr (StageShade<C>()) {
        if (S.n_lds_materials > 0) {
            uint4* dm = reinterpret_cast<uint4*>(rt_lds + lds_shade_offset<C>(S));
            const uint4* sm = reinterpret_cast<const uint4*>(S.materials);
            for (int i = threadIdx.x; i < S.n_lds_materials * 4; i += BlockThreads<C>()) dm[i] = sm[i];
            uint4* dt = dm + S.n_lds_materials * 4;
            const uint4* stx = reinterpret_cast<const uint4*>(S.textures);
            for (int i = threadIdx.x; i < S.n_lds_textures * 6; i += BlockThreads<C>()) dt[i] = stx[i];
            any = true;
        }
    }
    if (any) __syncthreads();
}

// One hit of ray_color (main.rs:25-34): emitted + attenuation * (next), with the
// recursion unrolled into the throughput T. A path carries at most one emission (a
// DiffuseLight ends it), so adding T*e straight into the chunk sum gives the same bits
// as the reference's per-sample sum. In three steps: shade_begin (emission; false if the
// path ends there), the material's draws (random_in_unit_sphere unless Dielectric), and
// shade_end (the scattered ray; false if Metal absorbs it). shade() runs them in a row; the
// pool schedules run the draws in one rejection loop with the camera's.
template <class C, class R = typename C::Real>
__device__ __forceinline__ bool shade_begin(const SceneDev& S, const HitT<R>& h, R Tr, R Tg, R Tb, double& sum_r,
                                            double& sum_g, double& sum_b)
{
    if (!S.has_lights) return true;   // wave-uniform: no material of the scene emits (no read needed)
    const rt_material& m = material_of<C>(S, h.mat);
    if (m.kind == RT_MAT_DIFFUSE_LIGHT) {  // material.rs:25-34 (emits on both faces, never scatters)
        R er, eg, eb;
        tex_value<C>(S, m.tex, h, er, eg, eb);
        sum_r = sum_r + (double)(Tr * er);   // the chunk sums stay f64 in the f32 mode too
        sum_g = sum_g + (double)(Tg * eg);
        sum_b = sum_b + (double)(Tb * eb);
        return false;
    }
    return true;
}
// whether the material draws a random_in_unit_sphere candidate (Lambertian, Metal, Isotropic)
template <class C>
__device__ __forceinline__ bool shade_draws(const SceneDev& S, int mat)
{
    return material_of<C>(S, mat).kind != RT_MAT_DIELECTRIC;
}
// (qx, qy, qz, l2): the material's random_in_unit_sphere draw (0, 0, 0, 1 for Dielectric)
template <class C, bool FIN = true, class R = typename C::Real>
__device__ __forceinline__ bool shade_end(const SceneDev& S, const HitT<R>& h, RayT<R>& r, rt_pstream& st, R& Tr,
                                          R& Tg, R& Tb, R qx, R qy, R qz, R l2)
{
    const rt_material& m = material_of<C>(S, h.mat);
    const int kind = m.kind;
    // The materials share their expensive steps, so a wave holding several materials runs
    // each once: one unit-sphere loop (Lambertian, Metal, Isotropic), one 1/sqrt (of the
    // candidate for Lambertian, of the ray direction for Metal and Dielectric), one texture
    // lookup (Lambertian, Isotropic).
    const R inv = (R)1 / r_sqrt(kind == RT_MAT_LAMBERTIAN ? l2 : r.a);
    R sdx, sdy, sdz, ar = (R)1, ag = (R)1, ab = (R)1;
    bool scattered = true;
    if (kind == RT_MAT_LAMBERTIAN) {  // material.rs:36-48
        sdx = h.nx + qx * inv;
        sdy = h.ny + qy * inv;
        sdz = h.nz + qz * inv;
        if (r_fabs(sdx) < (R)1e-8 && r_fabs(sdy) < (R)1e-8 && r_fabs(sdz) < (R)1e-8) {
            sdx = h.nx; sdy = h.ny; sdz = h.nz;
        }
    } else if (kind == RT_MAT_METAL || kind == RT_MAT_DIELECTRIC) {
        const R ux = r.dx * inv, uy = r.dy * inv, uz = r.dz * inv;  // normalize(r_in.direction)
        if (kind == RT_MAT_METAL) {  // material.rs:50-60
            const R fuzz = (R)m.fuzz;
            const R k2 = (R)2 * (ux * h.nx + uy * h.ny + uz * h.nz);
            sdx = (ux - h.nx * k2) + qx * fuzz;
            sdy = (uy - h.ny * k2) + qy * fuzz;
            sdz = (uz - h.nz * k2) + qz * fuzz;
            scattered = sdx * h.nx + sdy * h.ny + sdz * h.nz > (R)0;
            ar = (R)m.albedo[0]; ag = (R)m.albedo[1]; ab = (R)m.albedo[2];
        } else {  // material.rs:62-82, 89-94
            const R ir = (R)m.ir;
            const R ratio = h.front ? ((R)1 / ir) : ir;
            const R cos_theta = r_fmin((-ux) * h.nx + (-uy) * h.ny + (-uz) * h.nz, (R)1);
            const R sin_theta = r_sqrt((R)1 - cos_theta * cos_theta);
            const bool cannot_refract = ratio * sin_theta > (R)1;
            bool reflect = cannot_refract;
            if (!reflect) {  // the draw is skipped on TIR (the || short-circuit of material.rs:72)
                R r0 = ((R)1 - ratio) / ((R)1 + ratio);
                r0 = r0 * r0;
                const R refl = r0 + ((R)1 - r0) * r_pow5((R)1 - cos_theta);
                reflect = refl > draw_unit(st, (R)0);
            }
            if (reflect) {
                const R k2 = (R)2 * (ux * h.nx + uy * h.ny + uz * h.nz);
                sdx = ux - h.nx * k2;
                sdy = uy - h.ny * k2;
                sdz = uz - h.nz * k2;
            } else {  // math.rs:110-117 (cos_theta recomputed there from the same inputs)
                const R px = (ux + h.nx * cos_theta) * ratio;
                const R py = (uy + h.ny * cos_theta) * ratio;
                const R pz = (uz + h.nz * cos_theta) * ratio;
                const R pl = px * px + py * py + pz * pz;
                const R kk = -r_sqrt(r_fabs((R)1 - pl));
                sdx = px + h.nx * kk;
                sdy = py + h.ny * kk;
                sdz = pz + h.nz * kk;
            }
        }
    } else {  // isotropic, material.rs:84-87
        sdx = qx; sdy = qy; sdz = qz;
    }
    if (!scattered) return false;  // emitted (0) only
    if (kind == RT_MAT_LAMBERTIAN || kind == RT_MAT_ISOTROPIC) tex_value<C>(S, m.tex, h, ar, ag, ab);
    Tr = Tr * ar;
    Tg = Tg * ag;
    Tb = Tb * ab;
    r.ox = h.px; r.oy = h.py; r.oz = h.pz;
    if constexpr (C::F32) {
        // f32 mode: the hit point carries ~|p| 2^-24 of rounding, which t_min = 0.001 does not
        // cover at grazing angles on the final scene's |p| ~ 1000 boxes (the next ray would hit
        // its own surface again); move the origin off the surface, to the side the new ray
        // leaves on (Wachter & Binder, Ray Tracing Gems ch. 6). Media (uvkind 0) have no surface.
        // The scale is measured (round 6, C4 geometry at 16 spp, count variant; f64 paths: 3.690
        // casts per sample, 9.75 node visits per cast): |p| 2^-23 4.44 / 11.88, 2^-21 4.33 /
        // 11.85, 2^-19 (rounds 3-5) 4.14 / 11.64, 2^-17 3.93 / 10.85, 2^-15 3.696 / 9.72, 2^-13
        // 3.693 / 9.53 (profiles/r06m_*, r06n_*, r06o_*). Below 2^-15 the f32 paths re-hit their
        // own surfaces and run longer than the reference's; 2^-15 gives its path lengths (and
        // the statistical parity of tests/test_gpu_f32.py), 2^-13 starts to skip geometry.
        if (h.uvkind != 0) {
            const float m = fmaxf(fmaxf(__builtin_fabsf(h.px), __builtin_fabsf(h.py)), __builtin_fabsf(h.pz));
            float eps = m * 0x1.0p-15f + 1e-5f;
            if (sdx * h.nx + sdy * h.ny + sdz * h.nz < 0.0f) eps = -eps;
            r.ox = h.px + h.nx * eps;
            r.oy = h.py + h.ny * eps;
            r.oz = h.pz + h.nz * eps;
        }
    }
    r.dx = sdx; r.dy = sdy; r.dz = sdz;
    if constexpr (FIN) finish_ray<C>(r, S.has_spheres != 0);   // else the caller's trace step does it
    return true;
}
template <class C, bool FIN = true, class R = typename C::Real>
__device__ __forceinline__ bool shade(const SceneDev& S, const KParams& P, const HitT<R>& h, RayT<R>& r,
                                      rt_pstream& st, R& Tr, R& Tg, R& Tb, double& sum_r, double& sum_g,
                                      double& sum_b)
{
    if (!shade_begin<C>(S, h, Tr, Tg, Tb, sum_r, sum_g, sum_b)) return false;
    R qx = (R)0, qy = (R)0, qz = (R)0, l2 = (R)1;
    if (shade_draws<C>(S, h.mat)) random_in_unit_sphere(st, (R)P.scale_m11, qx, qy, qz, l2);
    return shade_end<C, FIN>(S, h, r, st, Tr, Tg, Tb, qx, qy, qz, l2);
}

}  // namespace rtk
