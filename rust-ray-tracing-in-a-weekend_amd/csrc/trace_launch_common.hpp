// trace_launch_common.hpp — what every launcher of the megakernel's device code shares: the launch
// record, the occupancy queries, the shape a scene and its options run (launch_shapes.hpp,
// KernelShape) with its dynamic LDS, the static-LDS guard of the 16-bit stack, and the one
// dispatcher from a shape onto the Cfg types. The trace launcher (trace_launch.hpp) and
// rt_render_features' launcher (features_device.hpp) are built from these pieces; this header
// names no kernel.
#pragma once
#include "trace_types.hpp"

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
    bool primary = false;          // KParams.primary is set (LaunchOpts.primary)
    bool defer_roots = false;      // with it: the CfgDefer kernels (LaunchOpts.defer_roots)
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

}  // namespace rtk
