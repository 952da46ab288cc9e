// trace_launch.hpp — the host side of a trace launch: which instantiation of the megakernel
// (trace_device.hpp: trace_chunks.hpp, trace_pool.hpp) a scene and its options run, with what
// workgroup, grid and dynamic LDS. The shape is resolved once (launch_shapes.hpp, KernelShape) and
// mapped onto the Cfg type by one dispatcher (trace_launch_common.hpp, which rt_render_features'
// launcher shares). Included by the translation units that launch trace kernels: trace_v_*.hip,
// trace_f32_*.hip and the dispatching trace_kernel.hip.
#pragma once
#include "trace_device.hpp"
#include "trace_launch_common.hpp"

namespace rtk {

// One feature set's kernels — f64 timed or counting, or the f32 fast mode's — one translation unit
// per instantiation (trace_v_*.hip, trace_f32_*.hip). Variant table: feature set x slab precision
// x stack x TLAS.
template <uint32_t F, bool COUNT, bool F32 = false>
hipError_t launch_variant(const Launch& L, const LaunchOpts& o, hipStream_t stream)
{
    const SceneDev& S = *L.S;
    KernelShape k = launch_shape(F, F32, S, o);
    if constexpr (!F32) {   // (the f64 kernels: the f32 mode's were never queried)
        if (k.s16) {
            using C = Cfg<F, true, true, true, COUNT, false>;
            static const bool static_lds =
                any_static_lds({(const void*)trace_pool<C, false>, (const void*)trace_pool<C, true>,
                                (const void*)trace_pool<C, false, true>, (const void*)trace_chunks<C>}) ||
                [] {   // the staged per-sample pool kernels
                    if constexpr (RT_STAGE_SEEDS != 0 && C::SHAPE.s16)
                        return any_static_lds({(const void*)trace_pool<CfgStage<C>, false>, (const void*)trace_pool<CfgStage<C>, false, true>});
                    else return false;
                }() ||
                [] {   // and their primary-candidate forms (timed kernels only)
                    if constexpr (RT_STAGE_SEEDS != 0 && C::SHAPE.s16 && F == FEAT_SET_SPHERES && !COUNT)
                        return any_static_lds({(const void*)trace_pool<CfgPrimary<C>, false>, (const void*)trace_pool<CfgPrimary<C>, false, true>});
                    else return false;
                }() ||
                [] {   // and those with deferred sphere roots
                    if constexpr (RT_STAGE_SEEDS != 0 && C::SHAPE.s16 && F == FEAT_SET_SPHERES && !COUNT)
                        return any_static_lds({(const void*)trace_pool<CfgDefer<C>, false>, (const void*)trace_pool<CfgDefer<C>, false, true>});
                    else return false;
                }();
            if (static_lds) k = without_stack16(k);
        }
    }
    const int bt = k.block_threads, wpb = bt / 64;
    // wave-wide sample starts (RT_STAGE_SEEDS): the plan's bytes for this launch pick the per-sample
    // pool's staged instantiation, which exists for the f64 16-bit-stack spheres kernels only
    const int seed_bytes = RT_STAGE_SEEDS && k.s16 && !F32 && L.pool == 1 && S.seed_stage_bytes == (int)seed_stage_bytes_of(bt)
                               ? S.seed_stage_bytes : 0;
    const size_t lds = launch_lds_bytes(k, S, seed_bytes);
    with_cfg<F, COUNT, F32>(k, [&](auto whole, auto part) {
        using C1 = decltype(whole);
        using C0 = decltype(part);
        if (L.pool) {
            auto go = [&](auto kernel) {
                unsigned nb = std::min<unsigned long long>(resident_blocks(L, kernel, lds, bt), (L.n_blocks + wpb - 1) / wpb);
                if (L.max_waves) nb = std::max(1u, std::min(nb, L.max_waves / (unsigned)wpb));
                hipLaunchKernelGGL(kernel, dim3(nb), dim3(bt), lds, stream, S, L.P, L.out, L.counters, L.work);
            };
            if constexpr (RT_STAGE_SEEDS != 0 && C1::SHAPE.s16 && !F32 && F == FEAT_SET_SPHERES && !COUNT) {
                if (seed_bytes && L.primary && L.defer_roots)
                    return go(L.max_waves ? trace_pool<CfgDefer<C1>, false, true> : trace_pool<CfgDefer<C1>, false>);
                if (seed_bytes && L.primary)
                    return go(L.max_waves ? trace_pool<CfgPrimary<C1>, false, true> : trace_pool<CfgPrimary<C1>, false>);
            }
            if constexpr (RT_STAGE_SEEDS != 0 && C1::SHAPE.s16 && !F32) {
                if (seed_bytes) return go(L.max_waves ? trace_pool<CfgStage<C1>, false, true> : trace_pool<CfgStage<C1>, false>);
            }
            if (L.pool == 2) go(k.nall ? trace_pool<C1, true> : trace_pool<C0, true>);
            else if (L.max_waves)   // the per-sample pool reducing in the kernel (KParams.ring)
                go(k.nall ? trace_pool<C1, false, true> : trace_pool<C0, false, true>);
            else go(k.nall ? trace_pool<C1, false> : trace_pool<C0, false>);
            return;
        }
        const auto kernel = k.nall ? trace_chunks<C1> : trace_chunks<C0>;
        if (L.waves_per_simd) (void)blocks_per_cu(L, kernel, lds, bt);
        hipLaunchKernelGGL(kernel, dim3((unsigned)((L.n_blocks + wpb - 1) / wpb)), dim3(bt), lds, stream, S, L.P, L.out, L.counters);
    });
    return hipGetLastError();
}

#define RT_VARIANT_DECL(F, COUNT, F32) \
    extern template hipError_t launch_variant<F, COUNT, F32>(const Launch&, const LaunchOpts&, hipStream_t);
RT_VARIANT_DECL(FEAT_SET_SPHERES, false, false)
RT_VARIANT_DECL(FEAT_SET_SPHERES, true, false)
RT_VARIANT_DECL(FEAT_SET_RECTINST, false, false)
RT_VARIANT_DECL(FEAT_SET_RECTINST, true, false)
RT_VARIANT_DECL(FEAT_SET_MEDIA, false, false)
RT_VARIANT_DECL(FEAT_SET_MEDIA, true, false)
RT_VARIANT_DECL(FEAT_SET_FINAL, false, false)
RT_VARIANT_DECL(FEAT_SET_FINAL, true, false)
RT_VARIANT_DECL(FEAT_ALL, false, false)
RT_VARIANT_DECL(FEAT_ALL, true, false)
RT_VARIANT_DECL(FEAT_SET_SPHERES, false, true)
RT_VARIANT_DECL(FEAT_SET_RECTINST, false, true)
RT_VARIANT_DECL(FEAT_SET_MEDIA, false, true)
RT_VARIANT_DECL(FEAT_SET_FINAL, false, true)
RT_VARIANT_DECL(FEAT_ALL, false, true)
// the f32 mode's count_work variants (final scene and spheres: the f32-vs-f64 path-length and
// step-cost comparison of DESIGN.md §5.6; trace_f32_*_count.hip)
RT_VARIANT_DECL(FEAT_SET_SPHERES, true, true)
RT_VARIANT_DECL(FEAT_SET_FINAL, true, true)
#undef RT_VARIANT_DECL

}  // namespace rtk
