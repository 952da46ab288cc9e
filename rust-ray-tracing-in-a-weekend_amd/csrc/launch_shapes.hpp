// launch_shapes.hpp — the shapes a trace launch and the host's launch plan must agree on:
// workgroup sizes per kernel variant, the Stack16 launch test, the in-kernel reduction's ring and
// the per-sample buffer's record count. No HIP: shared by the kernels (through trace_kernel.hpp),
// the plan (launch_plan.cpp) and CPU tests.
#pragma once

#include <cstddef>
#include <cstdint>

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

// workgroup threads of a kernel variant (host and device): see RT_BLOCK_FINAL, RT_BLOCK_SPHERES,
// RT_BLOCK_F32_SPHERES. s16: the spheres variant's 16-bit-stack configuration (slab32, LDS stack,
// whole TLAS in LDS: Stack16Cfg), the one those workgroup sizes and their wave counts are for;
// its other configurations keep 256-thread workgroups
#ifndef RT_STACK16
#define RT_STACK16 1
#endif
RT_LS_HD constexpr int block_threads_of(uint32_t variant_features, bool f32, bool s16 = false)
{
    return variant_features == 287u /* FEAT_SET_FINAL */            ? (f32 ? RT_BLOCK_F32_FINAL : RT_BLOCK_FINAL)
           : variant_features == 0u /* FEAT_SET_SPHERES */ && s16 ? (f32 ? RT_BLOCK_F32_SPHERES : RT_BLOCK_SPHERES)
                                                                   : 256;
}
// block_threads_of's s16 for a launch, from what the host knows of it: f32 slabs, the stack in
// LDS, the whole TLAS staged, and stack entries that fit 16 bits (SceneDev.stack16_ok; a scene
// whose entries do not fit takes the partial-TLAS instantiation). trace_device.hpp's launch code
// (launch_f, f32_nall, launch_one) reaches the same value in steps, through the NALL instantiation
// it picks; the two must agree, or the plan's workgroup size is not the launched kernel's.
RT_LS_HD constexpr bool stack16_launch(bool slab32, bool lds_stack, int n_lds_nodes, int n_tlas_nodes, bool stack16_ok)
{
    return RT_STACK16 && slab32 && lds_stack && n_lds_nodes > 0 && n_lds_nodes == n_tlas_nodes && stack16_ok;
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

// the per-sample buffer's records per sample: whole 8x8 tiles (trace_kernel.hpp, tiled_record)
RT_LS_HD inline size_t tiled_pixels(int width, int n_rows)
{
    return (size_t)((width + 7) / 8) * (size_t)((n_rows + 7) / 8) * 64;
}

}  // namespace rtk
