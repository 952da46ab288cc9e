// features_device.hpp — rt_render_features' kernel (include/rt/rt_abi.h): the first hit's albedo,
// normal and depth per (pixel, sample), over the megakernel's device functions (trace_shade.hpp and
// the layers below it: camera_ray, trace_world, tex_value, stage_lds; trace_grid.hpp: lane_work).
// It includes neither schedule (trace_chunks.hpp, trace_pool.hpp). Only the features_v_*.hip
// translation units and features_kernel.hip include it; the trace variants (trace_v_*.hip,
// trace_f32_*.hip) hold none of it.
//
// trace_chunks' layout without its bounce loop: one wave owns one 8x8 tile x one chunk of samples,
// one lane one pixel. Per sample the lane seeds the path stream and shoots the primary ray exactly
// as rt_render does for (pixel, sample) — ds_start, camera_ray with its jitter, lens and time
// draws — and makes one trace_world call with key.bounce = 0, so the medium's keyed draw decides a
// fog hit as rt_render's first bounce does. Nothing scatters and no further value is drawn. The
// lane adds the sample's seven values (albedo rgb, normal xyz, depth) to its chunk sums, each from
// 0.0 in sample order, and writes one 7-double partial per (pixel, chunk): reduce_features
// (features_kernel.hip) adds the partials in chunk order. Plain vector stores, no atomics.
//
// Launch bounds, waves per SIMD and the LDS layout are the trace kernel's of the same
// configuration (Cfg::SHAPE, lds_layout), so a scene's LDS plan serves both. The
// walk (trace_world) sets the register pressure, not the loop around it: each variant compiles to
// its trace_chunks twin's VGPR count, with about the same few dwords of scratch where that one
// has them (the compiler's figures: DESIGN.md §5.10).
#pragma once
#include "trace_shade.hpp"
#include "trace_grid.hpp"
#include "trace_launch_common.hpp"
#include "features_kernel.hpp"

namespace rtk {

template <class C>
__global__ void __launch_bounds__(BlockThreads<C>(), min_waves<C>()) trace_features(SceneDev S,
                                                                                   const KParams* __restrict__ Pp,
                                                                                   double* __restrict__ partial)
{
    static_assert(!C::F32 && !C::COUNT, "the feature pass is f64 and does not count work");
    const KParams& P = *Pp;
    stage_lds<C>(S);   // every thread of the block takes part, before any early return
    LaneWork w;
    if (!lane_work(P, w)) return;
    StackT<C> stack;
    if constexpr (Stack16Cfg<C>()) stack.base = reinterpret_cast<short*>(rt_lds + lds_stack_offset<C>(S)) + threadIdx.x;
    else if constexpr (C::LDS) stack.init((int)lds_stack_offset<C>(S));
    Count cnt{};
    double ar = 0.0, ag = 0.0, ab = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, dz = 0.0;
    Keyed key{P.seed, w.pixel, 0, 0};   // bounce 0: the primary ray's cast
    for (int s = w.s_begin; s < w.s_end; ++s) {
        rt_pstream st;
        ds_start(st, P.seed, w.pixel, (uint32_t)s);
        key.sample = (uint32_t)s;
        RayT<double> r;
        camera_ray(P, w.ix, w.y, st, r);
        finish_ray<C>(r, S.has_spheres != 0);
        HitT<double> h;
        if (!trace_world<C>(S, r, h, stack, key, cnt)) {   // a miss: the background, no normal, depth 0
            ar = ar + P.bg[0];
            ag = ag + P.bg[1];
            ab = ab + P.bg[2];
            continue;
        }
        const rt_material& m = material_of<C>(S, h.mat);
        const int kind = m.kind;
        double cr = 1.0, cg = 1.0, cb = 1.0;   // Dielectric: its attenuation
        if (kind == RT_MAT_METAL) {
            cr = m.albedo[0]; cg = m.albedo[1]; cb = m.albedo[2];
        } else if (kind != RT_MAT_DIELECTRIC) {   // Lambertian, Isotropic: the attenuation; DiffuseLight: the emission
            tex_value<C>(S, m.tex, h, cr, cg, cb);
        }
        ar = ar + cr;
        ag = ag + cg;
        ab = ab + cb;
        nx = nx + h.nx;
        ny = ny + h.ny;
        nz = nz + h.nz;
        const double ex = h.px - r.ox, ey = h.py - r.oy, ez = h.pz - r.oz;
        dz = dz + __builtin_sqrt((ex * ex + ey * ey) + ez * ez);
    }
    double* o = partial + (((size_t)w.chunk * P.n_rows + w.k) * P.width + w.x) * kFeatureChannels;
    o[0] = ar; o[1] = ag; o[2] = ab;
    o[3] = nx; o[4] = ny; o[5] = nz;
    o[6] = dz;
}

// One feature set's kernels (features_v_*.hip instantiate one each): launch_variant's shape — whole
// or partial TLAS in LDS, 16-bit stack entries only where they fit and the kernel has no static LDS
// in front of the node records — and its chunk-schedule launch (the same workgroup, the same
// dynamic LDS) for trace_features.
template <uint32_t F>
hipError_t launch_features_variant(const Launch& L, const LaunchOpts& o, hipStream_t stream)
{
    const SceneDev& S = *L.S;
    KernelShape k = launch_shape(F, false, S, o);
    if (k.s16) {
        static const bool static_lds = any_static_lds({(const void*)trace_features<Cfg<F, true, true, true, false, false>>});
        if (static_lds) k = without_stack16(k);
    }
    const int bt = k.block_threads, wpb = bt / 64;
    const size_t lds = launch_lds_bytes(k, S);
    const unsigned nb = (unsigned)((L.n_blocks + wpb - 1) / wpb);
    with_cfg<F, false, false>(k, [&](auto whole, auto part) {
        const auto kernel = k.nall ? trace_features<decltype(whole)> : trace_features<decltype(part)>;
        if (L.waves_per_simd) (void)blocks_per_cu(L, kernel, lds, bt);
        hipLaunchKernelGGL(kernel, dim3(nb), dim3(bt), lds, stream, S, L.P, L.out);
    });
    return hipGetLastError();
}
#define RT_FEATURES_DECL(F) \
    extern template hipError_t launch_features_variant<F>(const Launch&, const LaunchOpts&, hipStream_t);
RT_FEATURES_DECL(FEAT_SET_SPHERES)
RT_FEATURES_DECL(FEAT_SET_RECTINST)
RT_FEATURES_DECL(FEAT_SET_MEDIA)
RT_FEATURES_DECL(FEAT_SET_FINAL)
RT_FEATURES_DECL(FEAT_ALL)
#undef RT_FEATURES_DECL

}  // namespace rtk
