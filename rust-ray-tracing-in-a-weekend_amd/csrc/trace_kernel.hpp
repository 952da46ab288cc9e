// trace_kernel.hpp — launch interface of the megakernel (trace_kernel.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "rt/rt_scene.h"
#include "scene_features.hpp"   // FEAT_*, variant_features, RT_DEFER_INST
#include "launch_shapes.hpp"    // KernelShape, lds_layout, RT_BLOCK_*, block_threads_of, the ring's constants, tiled_pixels

namespace rtk {

// Device view of the uploaded rt_scene_soa tables.
struct SceneDev {
    const rt_prim* prims;
    const int32_t* prim_refs;
    const rt_prim* leaf_prims;  // prims[prim_refs[j]] for every leaf slot j (copied at upload):
                                // a primitive test reads its record directly, not through prim_refs
    const rt_bvh_node* nodes;
    const rt_instance* instances;
    const rt_material* materials;
    const rt_texture* textures;
    const double* perlin_ranvec;
    const int32_t* perlin_perm;
    const uint8_t* image;
    int32_t tlas_root;
    int32_t blas_base;      // first stack entry of a BLAS walk nested in the top-level walk
    int32_t stack_entries;  // traversal stack entries per lane (TLAS + nested BLAS walk, or the
                            // larger of the two when every BLAS walk is a deferred one: scene_lower.cpp)
    int32_t n_lds_nodes;    // the first n TLAS nodes (BFS order, nodes[0, n)) are copied into LDS
    int32_t n_tlas_nodes;   // TLAS size (its nodes are nodes[0, n_tlas_nodes))
    int32_t has_spheres;    // any Sphere / MovingSphere: rays need 1/|d|^2 for the root divisions
    int32_t has_lights;     // any DiffuseLight material (else no hit emits: the random scene)
    int32_t n_lds_materials;  // > 0: the material and texture tables are staged in LDS after the
    int32_t n_lds_textures;   // TLAS nodes (the kernel variants with rects or media; small tables)
    // A leaf the cast tests before the TLAS walk (0: none): a root child holding a primitive
    // far larger than the rest of the scene (the random scene's r = 1000 ground, the final
    // scene's r = 5000 fog), whose test then runs once per cast with the whole wave instead
    // of whenever each lane's walk reaches it; the walk starts below the root with t_max from
    // it. Its (padded) box gates the test; the walk then starts at pre_root, the other root
    // child. Only the spheres variants use it (PreLeaf: elsewhere the extra inlined leaf code
    // costs the variant its occupancy); the others walk from tlas_root as before.
    int32_t pre_leaf, pre_root;
    float pre_lo[3], pre_hi[3];
    // the TLAS walk's stack entries fit 16 bits (Stack16: node records at LDS byte addresses
    // < 32 KB, i.e. <= 409 TLAS nodes, and leaf codes of <= 1023 leaf slots); set at upload
    int32_t stack16_ok;
    // BLAS nodes staged in LDS after the TLAS records (variants with instanced BLASes): the device
    // node array holds one instance BLAS's nodes in BFS order right after the TLAS prefix,
    // nodes[n_tlas_nodes, n_tlas_nodes + n_blas_bfs) (scene_lower.cpp), and a launch stages the first
    // n_lds_blas of them (its LDS budget): the nested walk's top levels then read LDS
    int32_t n_blas_bfs, n_lds_blas;
    // LDS bytes per workgroup of the wave-wide sample starts, after the rest of the layout (the host's
    // plan, rtp::Plan.seed_stage_bytes); > 0 launches trace_pool's staged instantiation, 0 (every
    // other kernel, or no room) the per-lane one. (In the slot of a former padding word: the
    // kernel-argument layout is the one the kernels were timed with.)
    int32_t seed_stage_bytes;
};

struct KParams {
    rt_camera cam;
    double bg[3];
    double scale_m11;   // rand UniformFloat::new_inclusive(-1, 1) scale
    double scale_time;  // rand UniformFloat::new_inclusive(time0, time1) scale
    double wm1, hm1;    // width - 1, height - 1 (the jitter divisors of main.rs:517-518)
    double inv_wm1, inv_hm1;  // 1 / (width - 1), 1 / (height - 1), correctly rounded
    uint64_t seed;
    int32_t width, height, spp, max_depth;   // width: of the shard's pixel grid (the image's, or a tile slab's)
    int32_t spp_chunk, n_chunks;
    int32_t row_begin, row_stride, n_rows;
    int32_t row_block_shift;    // rows in bands of 2^shift (rt_render_params.row_block); 0: single rows
    int32_t tiles_x, tiles_y;   // 8x8 pixel tiles over (width, n_rows)
    int32_t sample_begin;       // chunk c covers samples [sample_begin + c*spp_chunk, ..) up to spp
    int32_t block_chunks;       // item pool: chunks per work block (a block = one tile x this many chunks)
    int32_t block_samples;      // per-sample pool: samples per work block (one tile x this many samples)
    uint32_t n_work_blocks;     // pool schedules: tiles x sample groups of this launch (host-computed: in
                                // the kernel the division's VGPR result stayed live through the loop)
    int32_t img_width;          // the image's width (pixel keys)
    int32_t tile_shard;         // rt_render_params.tile_shard: grid tile m = the frame's tile at position
                                // row_begin + m*row_stride of tile_order (raster order if null)
    int32_t img_tiles_x;        // tiles per tile row of the image
    // tile shards: ty = t / img_tiles_x as umulhi(t, tile_div_magic), exact for every tile t of the
    // frame (host-checked: t * (magic * img_tiles_x - 2^32) < 2^32); 0: a plain division
    uint32_t tile_div_magic;
    int32_t ring_waves;         // per-sample pool, in-kernel reduction: waves the ring holds (0: off)
    double* ring;               // per-sample pool, in-kernel reduction: kPoolRing blocks of records per wave
    // tile shards: the frame's tile order (rt_ctx_set_tile_order), position -> raster tile; null: raster
    const uint32_t* tile_order;
    // pool schedules: work blocks dealt tile-major (all of a tile's sample groups, then the next
    // tile: set with a tile order, so the most expensive tiles are done first and entirely) rather
    // than group-major; deal_div = the block index's inner extent: tiles (group-major) or sample
    // (chunk) groups per tile (tile-major). 2, 3 (kDealOrdered, kDealMeasure below): tile-major
    // through a whole frame's deal table
    int32_t tile_major;
    uint32_t deal_div;
    // count_work renders (COUNT kernels): per raster tile of the image, the lane-cycles its samples took
    unsigned long long* tile_cost;
    // RT_OPT_PRIMARY_CANDIDATES (primary_candidates.hpp): per image pixel (y * img_width + x) the 16-byte
    // record of the primitives its primary rays can hit; read by trace_pool's CfgPrimary instantiations
    // only, which the launcher picks when this is set (LaunchOpts.primary). Last: no other field moves.
    const uint4* primary;
};

// KParams.tile_major beyond 1, whole-frame renders on the kernels that carry it (trace_pool,
// DealCfg): tile-major through the deal table that follows the launch's work counter in memory,
// work[kDealTable + position] = raster tile (records and the frame stay raster), and, measuring,
// per raster tile the wave cycles (s_memtime, mod 2^32) between a wave's block fetches, added up at
// work[kDealTable + tiles + tile]. They sit behind the counter, and the mode in tile_major,
// because the kernel holds both in registers anyway.
constexpr int32_t kDealOrdered = 2, kDealMeasure = 3;
constexpr unsigned kDealTable = 16;   // words from the counter to the table (the counter keeps its cache line)
// the kernel variants that carry it (trace_pool.hpp, DealCfg): the spheres variants. The others
// hold their block state at the SGPR limit (RingSgpr) and keep raster order.
constexpr bool deal_variant(uint32_t variant) { return variant == FEAT_SET_SPHERES; }

struct LaunchOpts {
    uint32_t features;  // scene features (FEAT_*)
    int slab32;         // conservative f32 slab tests
    int lds_stack;      // traversal stack in LDS (1) or scratch (0)
    int count;          // count_work variant
    int pool;           // RT_SCHED_*: 0 chunks, 1 per-sample pool (per-sample output), 2 item pool (partials)
    int f32;            // the f32 fast mode (RT_PREC_F32)
    int primary = 0;    // KParams.primary is set: the per-sample pool's primary-candidate kernel, where one exists
    int defer_roots = 0;  // RT_OPT_DEFER_ROOTS: with `primary`, the kernel whose sphere tests defer the exact root (CfgDefer)
    int* waves_per_simd = nullptr;  // out (optional): resident waves per SIMD of the launched trace kernel
};

// The count_work counters (LaunchOpts.count; u64 each), by slot: what the trace kernels' epilogues
// add to (trace_chunks the first 15 and the two ray-generation parts, trace_pool all of them) and
// rt_last_stats / rt_last_counters read back. include/rt/rt_abi.h documents the same list under
// rt_last_counters, by number: that is the public statement, and these are its names.
enum CounterSlot : int {
    kCtrCasts = 0,            // rays cast
    kCtrNodeVisits = 1,       // BVH nodes visited, per lane
    kCtrPrimTests = 2,        // primitive tests, per lane
    kCtrCyclesCamera = 3,     // wave-cycles: ray generation, all of it
    kCtrCyclesTrace = 4,      //   trace (pool kernels: from the ray set-up to the hit record)
    kCtrCyclesShade = 5,      //   shading
    kCtrWaveSteps = 6,        // bounce-loop iterations per wave, summed
    kCtrWaveNodeSteps = 7,    // node-visit iterations per wave, summed
    kCtrCyclesNodes = 8,      // wave-cycles: node loops of the top-level walk
    kCtrCyclesLeaves = 9,     //   its leaf tests
    kCtrWaveLeafSteps = 10,   // leaf-loop iterations per wave, summed
    kCtrCameraLanes = 11,     // lanes starting a sample,
    kCtrCameraSteps = 12,     //   and the wave iterations in which any did
    kCtrShadeLanes = 13,      // lanes shading a hit,
    kCtrShadeSteps = 14,      //   and the wave iterations in which any did
    // pool kernels only, wave-cycles per finer phase
    kCtrCyclesSetup = 15,     // ray set-up
    kCtrCyclesPre = 16,       // the walk's prologue (pre-leaf test)
    kCtrCyclesRecord = 17,    // the hit record
    kCtrCyclesMedia = 18,     // media, inside the leaf tests
    kCtrCyclesInstances = 19, // instances, inside the leaf tests
    kCtrCyclesRefill = 20,    // refill
    kCtrCyclesKernel = 21,    // the waves' lifetimes, summed
    kCtrCyclesDeferred = 22,  // deferred instance walks, after the top-level walk
    kCtrCyclesSeed = 23,      // ray generation's seeding + jitter
    kCtrCyclesTries = 24,     // ray generation's rejection loop
    kCtrLongestWave = 25,     // the longest wave lifetime
    kCtrWaves = 26,           // waves
    // pool kernels only, bounce-loop lane slots that cast nothing (with casts: 64 x wave_steps)
    kCtrIdleTail = 27,        // idle, no unit left to take (the launch's tail)
    kCtrIdleRing = 28,        // idle, every ring slot holding an unfinished block
    kCtrNoScatter = 29,       // the path ended in its scatter
    kCtrDepthCap = 30,        // the depth cap
    kCtrTryWait = 31,         // a rejection loop carried to the next iteration
};
constexpr int kCounters = kCtrTryWait + 1;
static_assert(kCounters == 32, "rt_last_counters documents 32 slots");

// Per-sample pool output: [8x8 tile][sample of the batch][64 pixels of the tile, row-major]
// radiance records (f64 x 3). A wave's work block is one tile x consecutive samples and its
// lanes take the block's units in order, so records written close in time lie close in memory
// and fill whole cache lines while those sit in L2; the earlier [sample][pixel] layout spread
// each (tile, sample)'s 64 records over 8 image rows written ~1 ms apart, and L2 evicted the
// lines half written (C2 DRAM writes 1.22x the radiance bytes, C4 1.29x; profiles/r03o_*).
// Edge tiles keep all 64 slots (unused ones are never written or read).
struct SampleTiles {
    int32_t width, n_rows, tiles_x;
    int32_t f32_records;   // the f32 mode's records: f32 x 3 (12 B) instead of f64 x 3 (24 B)
};
__host__ __device__ inline size_t tiled_record(int tiles_x, int n_samples, int x, int k, int s)
{
    const size_t tile = (size_t)(k >> 3) * (size_t)tiles_x + (size_t)(x >> 3);
    return (tile * (size_t)n_samples + (size_t)s) * 64 + (size_t)(((k & 7) << 3) | (x & 7));
}

// Ph: host copy of the params (grid size); P: the same params in device memory
// chunk schedule: out = chunk partials [n_chunks][n_px][3]; pool schedule: out = per-sample
// radiance, tiled_record order over spp - sample_begin samples; work = one device counter
hipError_t launch_trace(const SceneDev& S, const KParams& Ph, const KParams* P, double* out,
                        unsigned long long* counters, unsigned* work, const LaunchOpts& o, hipStream_t stream);
// the primary-candidate table of a camera and frame size over the uploaded scene (primary_candidates.hip):
// table = width x height 16-byte records, *flagged = the pixels flagged "walk"
hipError_t launch_primary_candidates(const SceneDev& S, const rt_camera& cam, int width, int height, int k_max, void* table,
                                     unsigned* flagged, hipStream_t stream);
// and the table's all-sky 8x8 raster tiles (RT_OPT_SKIP_SKY_TILES): flags = one byte per tile, *n_sky = how many are set
hipError_t launch_primary_sky_tiles(const void* table, int width, int height, uint8_t* flags, unsigned* n_sky,
                                    hipStream_t stream);
// RT_OPT_SKIP_SKY_TILES: the raster tiles the trace launch was not dealt (flags[tile] != 0; null:
// none) and what every sample record of theirs would hold (0.0 + 1.0 * background, per channel)
struct SkyTiles {
    const uint8_t* flags = nullptr;
    double rec[3] = {0.0, 0.0, 0.0};
};
// pool schedule: per pixel, chunk sums of its samples (sample order) added to 0.0, scaled to out
// (out and the carried sums are in pixel order k * width + x); a tile flagged in `sky` sums
// sky.rec in place of every record, addition for addition
hipError_t launch_reduce_samples(const double* samples, void* out, bool f64, SampleTiles g, int n_samples,
                                 int chunk, double scale, hipStream_t stream, const SkyTiles& sky = SkyTiles{});
// the same across buffer batches: acc = closed chunks' total, open = the chunk in progress
// (pos of its samples seen before this batch); close ends the last chunk
hipError_t launch_reduce_samples_carry(const double* samples, double* acc, double* open, SampleTiles g,
                                       int n_samples, int chunk, int pos, bool close, hipStream_t stream);
hipError_t launch_reduce(const double* partial, void* out, bool f64, long long n_px, int n_chunks, double scale,
                         hipStream_t stream);
// acc[i] += chunk partials in chunk order (progressive accumulation, rt_accum_add)
hipError_t launch_accumulate(const double* partial, double* acc, long long n_px, int n_chunks, hipStream_t stream);
// tile shards gathered from `world` ranks (rank r's slab at r * slab_elems elements) -> the frame
// (height x width x 3, row 0 = bottom) in the tile order `order` (null: raster); rt_tiles_assemble
hipError_t launch_assemble_tiles(const void* gathered, void* frame, bool f64, int world, long long slab_elems,
                                 int width, int height, const uint32_t* order, hipStream_t stream);
hipError_t launch_eval(int fn, const double* x, const double* y, const double* z, double* out, int n,
                       hipStream_t stream);

// Tile-adaptive sampling (rt_render_adaptive; adaptive_kernel.hip). The frame-layout accumulators
// of one call (row 0 = bottom, pixel y * width + x) and its tile order: the per-sample records of
// shard tile m belong to the raster tile order[pos_begin + m].
struct AdaptiveFrame {
    double* sum;        // height x width x 3: RGB sums of the closed chunks
    double* sum_open;   // height x width x 3: the chunk in progress between buffer batches
    double* q;          // height x width: sum of squared sample luminances, closed chunks
    double* q_open;     // height x width: the chunk in progress
    double* tile_error; // per raster tile: E_t after the tile's last pass
    uint32_t* tile_spp; // per raster tile: samples per pixel taken so far
    const uint32_t* order;
    int32_t width, height, tiles_x, pos_begin;
};
// rt_render_adaptive_halves: the RGB sums of the samples with an even (a) and with an odd (b)
// global sample index, summed as AdaptiveFrame::sum is and laid out like it. A struct of its own,
// passed to the moments kernel after its other arguments: rt_render_adaptive's instantiation takes
// the AdaptiveFrame it always took, at the same argument offsets.
struct AdaptiveHalves {
    double* sum_a;        // height x width x 3: closed chunks, even samples
    double* sum_a_open;   // height x width x 3: the chunk in progress between buffer batches
    double* sum_b;        // the same of the odd samples
    double* sum_b_open;
};
// a batch of n_samples records per pixel of the shard's n_tiles tiles (tiled_record order) added to
// the frame's moments; pos = samples of the open chunk seen before this batch; close: the pass's
// last batch (ends the chunk, writes tile_error / tile_spp = n_done for the shard's tiles).
// halves (null: rt_render_adaptive's kernel) also takes the two half sums; first = the global index
// of the batch's first sample, whose parity no chunk position gives when the chunk is odd.
hipError_t launch_adaptive_moments(const double* samples, const AdaptiveFrame& F, int n_tiles, int n_samples,
                                   int chunk, int pos, bool close, int n_done, hipStream_t stream,
                                   const AdaptiveHalves* halves = nullptr, int first = 0);
// mean (f32 / f64) = sum * (1 / tile_spp of the pixel's tile); se_map (may be null) = per-pixel se
hipError_t launch_adaptive_resolve(const double* sum, const double* q, const uint32_t* tile_spp, void* mean, bool f64,
                                   double* se_map, int width, int height, hipStream_t stream);
// mean_a = sum_a * (1 / n_a), mean_b = sum_b * (1 / n_b) (f32 / f64); n = tile_spp of the pixel's
// tile (>= 2), n_a = (n + 1) / 2, n_b = n / 2
hipError_t launch_adaptive_resolve_halves(const double* sum_a, const double* sum_b, const uint32_t* tile_spp,
                                          void* mean_a, void* mean_b, bool f64, int width, int height,
                                          hipStream_t stream);

}  // namespace rtk
