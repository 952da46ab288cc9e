// trace_launch.hpp — the host side of a trace launch: which instantiation of the megakernel
// (trace_device.hpp) a scene and its options run, with what workgroup, grid and dynamic LDS. The
// shape is resolved once (launch_shapes.hpp, KernelShape) and mapped onto the Cfg type by one
// dispatcher; rt_render_features' launcher (features_device.hpp) uses the same pieces. Included by
// the translation units that launch: trace_v_*.hip, trace_f32_*.hip, features_v_*.hip and the two
// dispatching ones (trace_kernel.hip, features_kernel.hip).
#pragma once
#include "trace_device.hpp"

namespace rtk {

struct Launch {
    const SceneDev* S;
    const KParams* P;
    double* out;                   // chunk partials (chunk schedule) or per-sample radiance (pool)
    unsigned long long* counters;
    unsigned* work;                // pool / items: work-block counter
    int pool;                      // 0 chunks, 1 per-sample pool, 2 item pool
    unsigned long long n_blocks;   // 8x8 tiles x chunks
    int* waves_per_simd;           // out (optional): resident blocks per CU = waves per SIMD (4-wave blocks)
    unsigned max_waves = 0;        // per-sample pool with the in-kernel reduction: waves its ring holds
};

// Resident blocks per CU of a kernel (registers, LDS); waves per SIMD reported to the caller.
template <class K>
static int blocks_per_cu(const Launch& L, K kernel, size_t lds, int bt)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, bt, lds) != hipSuccess || per_cu <= 0) per_cu = 1;
    if (L.waves_per_simd) *L.waves_per_simd = per_cu * (bt / 256);   // 4 SIMDs per CU
    return per_cu;
}

// Persistent grid for the pool schedule: as many blocks as fit on the device at once.
template <class K>
static unsigned resident_blocks(const Launch& L, K kernel, size_t lds, int bt)
{
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    }
    return (unsigned)(cus * blocks_per_cu(L, kernel, lds, bt));
}

// The shape a launch of feature set F runs (launch_shapes.hpp, launch_shape); the f32 mode's
// kernels test f32 slabs always (an f32 path gains nothing from f64 boxes)
inline KernelShape launch_shape(uint32_t F, bool f32, const SceneDev& S, const LaunchOpts& o)
{
    return launch_shape(F, f32 || o.slab32 != 0, o.lds_stack != 0, f32, S.n_lds_nodes, S.n_tlas_nodes, S.stack16_ok != 0);
}

// Its dynamic LDS: the scene's staged counts in the shape's layout, then the staged sample starts
inline size_t launch_lds_bytes(const KernelShape& k, const SceneDev& S, int seed_bytes = 0)
{
    const size_t rest = lds_layout(k, S.n_lds_nodes, S.n_lds_blas, S.stack_entries, S.n_lds_materials, S.n_lds_textures).total;
    return seed_bytes ? lds_seeds_offset(rest) + (size_t)seed_bytes : rest;
}

// stack16_ok (scene_lower.cpp) assumes the node records start at LDS address 0, i.e. that rt_lds is
// the kernels' only __shared__ object: a static __shared__ variable would move the dynamic base
// up, and 16-bit stack entries would truncate node addresses past 32 KB. Checked on the compiled
// kernels a 16-bit-stack launch can run: any static LDS in them sends the scene to the
// partial-TLAS, 32-bit-stack shape.
inline bool any_static_lds(std::initializer_list<const void*> kernels)
{
    hipFuncAttributes a;
    for (const void* k : kernels)
        if (hipFuncGetAttributes(&a, k) != hipSuccess || a.sharedSizeBytes != 0) return true;
    return false;
}
inline KernelShape without_stack16(const KernelShape& k) { return kernel_shape(k.features, k.s32, k.lds, false, k.f32); }

// The Cfg types of a shape of feature set F: fn gets, as values of those types, the instantiations of
// the shape's slab precision and stack with the whole TLAS in LDS (NALL) and without. The two have
// kernels of one signature, so k.nall picks between them as between two function pointers. (The
// f32 mode has no f64-slab kernels. A translation unit's code object holds its kernels in the order
// the launcher first names them, so reordering the names below moves code: scripts/device_code_hashes.py.)
template <uint32_t F, bool COUNT, bool F32, class Fn>
static void with_cfg(const KernelShape& k, Fn fn)
{
    if (k.s32) {
        if (k.lds) fn(Cfg<F, true, true, true, COUNT, F32>{}, Cfg<F, true, true, false, COUNT, F32>{});
        else fn(Cfg<F, true, false, true, COUNT, F32>{}, Cfg<F, true, false, false, COUNT, F32>{});
    } else if constexpr (!F32) {
        if (k.lds) fn(Cfg<F, false, true, true, COUNT, F32>{}, Cfg<F, false, true, false, COUNT, F32>{});
        else fn(Cfg<F, false, false, true, COUNT, F32>{}, Cfg<F, false, false, false, COUNT, F32>{});
    }
}

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
