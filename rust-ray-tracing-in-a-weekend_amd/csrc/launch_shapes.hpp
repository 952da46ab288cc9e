// launch_shapes.hpp — the shape of a trace launch, stated once: which Cfg<F, S32, LDS, NALL, COUNT,
// F32> instantiation runs (KernelShape), its workgroup size, its launch bound and its dynamic-LDS
// layout (lds_layout). The kernels read the shape of their configuration (trace_types.hpp, Cfg), the
// launchers resolve it from a scene and its options (trace_launch_common.hpp), the host's plan carries it
// (launch_plan.cpp). Also the in-kernel reduction's ring and the per-sample buffer's record
// count. No HIP: shared by the kernels (through trace_kernel.hpp), the plan and CPU tests.
#pragma once

#include <cstddef>
#include <cstdint>

#include "scene_features.hpp"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define RT_LS_HD __host__ __device__
#else
#define RT_LS_HD
#endif

// Threads per workgroup of the final-scene variant's kernels (the others: 256). 512 (8 waves)
// shares one LDS copy of the TLAS and materials among twice the waves, which leaves room for
// the instanced BLAS in LDS (SceneDev.n_lds_blas; the host sizes that budget with it): the
// final scene's 1000-sphere BLAS 512 of (then) 548 nodes staged instead of 64 (597 today), C4 1920x1080x100
// 110.95 -> 108.23 ms; 512 threads with 64 staged 111.27 (profiles/r03r_ab_c4.log)
// Round 6: 1024 (16 waves, one workgroup per CU at 4 waves per SIMD) stages the whole BLAS and
// shares one copy of everything among the CU's waves: C4 1920x1080x1000 979.1 -> 976.4 ms, f32 mode
// at 100 spp 86.33 -> 84.98, images bit-identical (profiles/r06u_ab_b1024_c4*.log; at 100 spp
// 105.15 -> 104.71, r06t_ab_b1024_c4.log)
#ifndef RT_BLOCK_FINAL
#define RT_BLOCK_FINAL 1024
#endif

namespace rtk {

// Threads per workgroup of the f32 mode's spheres variant: its 76 VGPRs allow 6 waves per SIMD,
// which 256-thread blocks cannot reach (each holds its own 22.7 KB copy of the random scene's
// TLAS, 6 x 28.8 KB > 160 KB per CU); 512-thread blocks share one copy among 8 waves (3 blocks,
// 105 KB).
#ifndef RT_BLOCK_F32_FINAL
#define RT_BLOCK_F32_FINAL RT_BLOCK_FINAL
#endif
// Threads per workgroup of the f64 spheres variant (C1, C2, C5): 768 (12 waves, two workgroups per
// CU) at 6 waves per SIMD (RT_MIN_WAVES_SPHERES_S16: 80 VGPRs, 32-40 B of scratch), two LDS copies
// of the TLAS per CU instead of five. C2 1200x800x500 74.55 -> 72.00 ms, images identical; 512
// threads at 6 waves 72.24, 384 at 6 81.12, 448 at 7 (96 B of scratch) 89.86, 512 at 5 (two
// workgroups: 4 waves per SIMD) 82.42 (profiles/r06w_ab_sph_c2.log, r06x_ab_sph_c2.log)
#ifndef RT_BLOCK_SPHERES
#define RT_BLOCK_SPHERES 768
#endif
#ifndef RT_BLOCK_F32_SPHERES
#define RT_BLOCK_F32_SPHERES 512
#endif

// 16-bit LDS stack entries in the spheres variant with the whole TLAS in LDS: its 35 KB of LDS
// per block (22.7 KB of node records + a 12-entry 32-bit stack) let only 4 blocks share a CU's
// 160 KB; with 6.1 KB of stack 5 blocks fit, and the variant runs at 5 waves per SIMD (96
// VGPRs, min_waves) — C2 1200x800x100 16.48 -> 15.40 ms, same bits (profiles/r02ao_*)
// (the final-scene variant with 16-bit entries measured ~7 % slower: C4 1920x1080x100 142.1 vs
// 132.7 ms, r03f_ab_c4.log; the spheres variant only)
#ifndef RT_STACK16
#define RT_STACK16 1
#endif
// the variants with nested walks stage BLAS nodes (SceneDev.n_lds_blas; the host sets it only for them)
#ifndef RT_STAGE_BLAS
#define RT_STAGE_BLAS 1
#endif

// Minimum waves per SIMD requested from the register allocator (the launch bound), per feature set
#ifndef RT_MIN_WAVES_F32_SPHERES
#define RT_MIN_WAVES_F32_SPHERES 6   // 76 VGPRs (<= 80 for 6), 512-thread blocks (RT_BLOCK_F32_SPHERES)
#endif
#ifndef RT_MIN_WAVES_SPHERES
#define RT_MIN_WAVES_SPHERES 1
#endif
// the f64 spheres variant with its 16-bit LDS stack (C1, C2, C5): 6 waves per SIMD at 80 VGPRs
// (94 at 5, spill-free) with 768-thread workgroups (RT_BLOCK_SPHERES)
#ifndef RT_MIN_WAVES_SPHERES_S16
#define RT_MIN_WAVES_SPHERES_S16 6
#endif
#ifndef RT_MIN_WAVES_RECTINST
// measured (Cornell 800x800x200): chunk schedule 4 waves 190 vs 202 ms; pool schedule 4: 80.7,
// 3: 81.0; after the reciprocal divisions (more live state, 4 waves spilled to scratch):
// 4: 66.6, 3: 58.6; round 2: without the nested BLAS walk (FEAT_INST_BLAS), the f64-slab
// instantiation the node-free Cornell scenes run needs 125 VGPRs: 4 waves at this bound
#define RT_MIN_WAVES_RECTINST 3
#endif
#ifndef RT_MIN_WAVES_ALL
// measured, pool schedule: final scene 960x540x200 4: 112.0 ms (scratch spills: 0.7 TB of HBM
// writes per launch), 3: 102.8, 2: 131.5; cornell smoke 600x600x200 4: 74.1, 3: 62.3, 2: 79.7
#define RT_MIN_WAVES_ALL 3
#endif
#ifndef RT_MIN_WAVES_MEDIA
#define RT_MIN_WAVES_MEDIA 3
#endif
#ifndef RT_MIN_WAVES_FINAL
// round 3: 4 (127 VGPRs, no spills, once machine LICM no longer pins the cold paths' f64
// constants in VGPRs and the hit record is dead during the walk); round 2 measured 3 best
// (4: 112.0 ms with 0.7 TB of scratch writes per launch, 3: 102.8, 2: 131.5 at 960x540x200)
#define RT_MIN_WAVES_FINAL 4
#endif
// the f32 final-scene variant: 4 like the f64 one (3 waves, 136-142 VGPRs and no spills even with
// the small-sphere test, is slower: C4 1920x1080x100 f32 101.9 ms with 768-thread blocks, 107.0
// with 256, against 89.4 at 4; profiles/r06s_ab_f32final_c4.log)
#ifndef RT_MIN_WAVES_F32_FINAL
#define RT_MIN_WAVES_F32_FINAL RT_MIN_WAVES_FINAL
#endif

// Bytes of the records a workgroup stages in LDS (trace_walk.hpp asserts them against the types):
// rt_bvh_node, the whole-TLAS f32-slab node LdsNode, rt_material, rt_texture. (A staged sample
// start's slot: kSeedSlotBytes below.)
constexpr size_t kBvhNodeBytes = 64, kLdsNodeBytes = 80, kMaterialBytes = 64, kTextureBytes = 96;

// What one Cfg<F, S32, LDS, NALL, COUNT, F32> instantiation launches as. The kernels read it as
// Cfg::SHAPE; launch_shape below resolves the same value from what the host knows of a launch.
struct KernelShape {
    uint32_t features;    // the variant's feature set (FEAT_SET_*, FEAT_ALL)
    bool s32, lds, nall, f32;   // Cfg's coordinates: f32 slabs, the stack in LDS, the whole TLAS in LDS, the f32 mode
    bool s16;             // 16-bit LDS stack entries (RT_STACK16): the spheres variant with f32 slabs, the
                          // LDS stack and the whole TLAS; the large workgroups and their wave counts are for it
    int block_threads;    // RT_BLOCK_FINAL, RT_BLOCK_SPHERES, RT_BLOCK_F32_*; 256 otherwise
    int node_bytes;       // a staged TLAS node: kLdsNodeBytes with the whole TLAS and f32 slabs, else kBvhNodeBytes
    int entry_bytes;      // an LDS stack entry
    bool stage_shade;     // small material and texture tables in LDS (the variants with rects or media; the
                          // random scene's 485 materials would cost the spheres variant blocks per CU)
    bool stage_blas;      // the instanced BLAS's top levels in LDS (RT_STAGE_BLAS)
    int min_waves;        // the launch bound: waves per SIMD (RT_MIN_WAVES_*)
};
RT_LS_HD constexpr bool operator==(const KernelShape& a, const KernelShape& b)
{
    return a.features == b.features && a.s32 == b.s32 && a.lds == b.lds && a.nall == b.nall && a.f32 == b.f32 &&
           a.s16 == b.s16 && a.block_threads == b.block_threads && a.node_bytes == b.node_bytes &&
           a.entry_bytes == b.entry_bytes && a.stage_shade == b.stage_shade && a.stage_blas == b.stage_blas &&
           a.min_waves == b.min_waves;
}
// from the template coordinates
RT_LS_HD constexpr KernelShape kernel_shape(uint32_t F, bool S32, bool LDS, bool NALL, bool F32)
{
    const bool spheres = F == FEAT_SET_SPHERES, final_ = F == FEAT_SET_FINAL;
    const bool s16 = RT_STACK16 && LDS && NALL && S32 && spheres;
    return KernelShape{F, S32, LDS, NALL, F32, s16,
                       final_ ? (F32 ? RT_BLOCK_F32_FINAL : RT_BLOCK_FINAL)
                       : s16  ? (F32 ? RT_BLOCK_F32_SPHERES : RT_BLOCK_SPHERES) : 256,
                       (int)(NALL && S32 ? kLdsNodeBytes : kBvhNodeBytes), s16 ? 2 : 4, !spheres,
                       RT_STAGE_BLAS && (F & FEAT_INST_BLAS) != 0,
                       s16 && F32              ? RT_MIN_WAVES_F32_SPHERES
                       : F32 && final_         ? RT_MIN_WAVES_F32_FINAL
                       : s16                   ? RT_MIN_WAVES_SPHERES_S16
                       : spheres               ? RT_MIN_WAVES_SPHERES
                       : F == FEAT_SET_RECTINST ? RT_MIN_WAVES_RECTINST
                       : F == FEAT_SET_MEDIA    ? RT_MIN_WAVES_MEDIA
                       : final_                 ? RT_MIN_WAVES_FINAL : RT_MIN_WAVES_ALL};
}
// from what the host knows of a launch: the variant, the context's switches as the plan resolved
// them (the f32 mode tests f32 slabs always: Plan.slab32 is 1 there), the TLAS nodes staged and
// present, and whether the scene's stack entries fit 16 bits (rtl::Lowered.stack16_ok). The whole
// TLAS in LDS is NALL, except that a spheres launch whose entries do not fit takes the
// partial-TLAS instantiation, which keeps 32-bit entries.
RT_LS_HD constexpr KernelShape launch_shape(uint32_t variant, bool slab32, bool lds_stack, bool f32, int n_lds_nodes,
                                            int n_tlas_nodes, bool stack16_ok)
{
    const bool narrow = RT_STACK16 && variant == FEAT_SET_SPHERES && slab32 && lds_stack;   // kernel_shape's s16, given NALL
    return kernel_shape(variant, slab32, lds_stack, n_lds_nodes > 0 && n_lds_nodes == n_tlas_nodes && !(narrow && !stack16_ok), f32);
}
// Two views of the shape for callers that hold a variant and its s16 apart (tests/seed_stage_dump.cpp):
// the workgroup threads of a variant in or out of its 16-bit-stack configuration, and whether a
// spheres launch is in it
RT_LS_HD constexpr int block_threads_of(uint32_t variant_features, bool f32, bool s16 = false)
{
    return kernel_shape(variant_features, s16, s16, s16, f32).block_threads;
}
RT_LS_HD constexpr bool stack16_launch(bool slab32, bool lds_stack, int n_lds_nodes, int n_tlas_nodes, bool stack16_ok)
{
    return launch_shape(FEAT_SET_SPHERES, slab32, lds_stack, false, n_lds_nodes, n_tlas_nodes, stack16_ok).s16;
}

// The block's dynamic LDS: [TLAS nodes][BLAS nodes][stack: entries x block lanes][materials][textures]
struct LdsLayout {
    size_t blas, stack, shade, total;   // byte offsets of the BLAS nodes, the stack and the material table; bytes
};
RT_LS_HD constexpr LdsLayout lds_layout(int n_nodes, int node_bytes, int n_blas, int stack_entries,
                                        int entry_bytes, int n_materials, int n_textures, int lanes)
{
    const size_t blas = (size_t)n_nodes * (size_t)node_bytes;
    const size_t stack = blas + (size_t)n_blas * kBvhNodeBytes;
    const size_t shade = stack + (size_t)stack_entries * (size_t)lanes * (size_t)entry_bytes;
    return LdsLayout{blas, stack, shade, shade + (size_t)n_materials * kMaterialBytes + (size_t)n_textures * kTextureBytes};
}
// a shape's layout of a scene's staged counts (SceneDev's fields of these names): the shape says
// which of them its kernels stage
RT_LS_HD constexpr LdsLayout lds_layout(const KernelShape& k, int n_lds_nodes, int n_lds_blas, int stack_entries,
                                        int n_lds_materials, int n_lds_textures)
{
    return lds_layout(n_lds_nodes, k.node_bytes, k.stage_blas ? n_lds_blas : 0, k.lds ? stack_entries : 0, k.entry_bytes,
                      k.stage_shade ? n_lds_materials : 0, k.stage_shade ? n_lds_textures : 0, k.block_threads);
}

// Per-sample pool with the reduction in the kernel (round 5): a wave's work block (one tile x
// one chunk of samples) is owned by that wave alone, so the wave counts its finished samples
// and, when the block's last one ends, sums every pixel's samples in order and writes the
// chunk partial (reduce_chunks' input). The records wait in a ring of kPoolRing blocks per
// wave (record j of a block: sample j / 64, pixel j % 64 of the 8x8 tile). Needs chunks of at
// most 16 samples and samples below 2^20 (the host checks both).
constexpr int kPoolRing = 4;
constexpr unsigned kRingSlot = 16 * 64;        // records per ring slot: chunks of at most 16 samples
constexpr int kRingCur = kPoolRing;            // lanes of the wave's ring-state VGPR (trace_pool):
constexpr int kRingOcc = kPoolRing + 1;        //   the slot units are taken from, the occupied slots
constexpr size_t kRingWaveDoubles = (size_t)kPoolRing * kRingSlot * 3 + 8;   // a wave's records + header
constexpr int kRingSampleBits = 20;            // ring: samples below 2^20, the record index above
constexpr uint32_t kRingSampleMask = (1u << kRingSampleBits) - 1;
static_assert(kPoolRing * kRingSlot <= (1u << (32 - kRingSampleBits)), "ring record index bits");

// Wave-wide sample starts (trace_pool's staged instantiations): units of a work
// block are dealt sample-major, so the 64 samples a wave starts next are always one sample of its
// tile's 64 pixels. The wave seeds and jitters that whole row at once — lane p pixel p — into a
// staging area of its own in LDS (kSeedSlotBytes per pixel: the path stream after the jitter
// draws, then u and v), and a lane that takes a unit reads its slot, instead of the ~22 lanes
// that start a sample in a bounce-loop iteration running the sequence under their exec mask.
// The f64 spheres variant's 16-bit-stack per-sample pool kernels only (buffer and ring forms);
// the host's plan decides per launch (rtp::Plan.seed_stage_bytes). 0: compiled out (A/B builds).
// C2 1200x800x500 against the parent commit's library, 18 renders each: 70.39 -> 68.14 ms, every
// frame identical; the count variant's "seeding + jitter" share 0.067 -> 0.019 of wave time, the
// refill's 0.140 -> 0.166 (profiles/staged_seeds_ab_c2.log, staged_seeds_phases_c2.log).
#ifndef RT_STAGE_SEEDS
#define RT_STAGE_SEEDS 1
#endif
constexpr size_t kSeedSlotBytes = 32;
RT_LS_HD constexpr size_t seed_stage_bytes_of(int block_threads) { return kSeedSlotBytes * (size_t)block_threads; }
// The slots follow the rest of the layout on a boundary of their size: their byte offset from the
// layout's total. (A function of its own: lds_layout is inlined by cost, and the kernels that do
// not stage keep their code.)
RT_LS_HD constexpr size_t lds_seeds_offset(size_t layout_total) { return (layout_total + kSeedSlotBytes - 1) / kSeedSlotBytes * kSeedSlotBytes; }

// the per-sample buffer's records per sample: whole 8x8 tiles (trace_kernel.hpp, tiled_record)
RT_LS_HD inline size_t tiled_pixels(int width, int n_rows)
{
    return (size_t)((width + 7) / 8) * (size_t)((n_rows + 7) / 8) * 64;
}

}  // namespace rtk
