// launch_plan.cpp — see launch_plan.hpp. Every branch here carries the measurement that put it
// there; the numbers are kernel (+ reduce) ms per frame on the MI355X, the logs under profiles/.
#include "launch_plan.hpp"

#include <algorithm>
#include <cmath>

#include "launch_shapes.hpp"
#include "scene_features.hpp"

namespace rtp {

namespace {

// LDS stack entries per lane above which the scratch stack is used (48 KB per block)
constexpr int kMaxLdsStack = 48;
// TLAS nodes kept in LDS (32 KB per block): the first kMaxLdsNodes in BFS order, i.e.
// the top levels; deeper ones are read from L1/L2
constexpr int kMaxLdsNodes = 512;
// instance BLAS nodes staged in LDS at most
#ifndef RT_LDS_BLAS_MAX
#define RT_LDS_BLAS_MAX 1024   // the LDS budget decides (512-thread final variant: 512 of the final scene's then 548
                               // BLAS nodes, 110.95 -> 108.23 ms at C4 1920x1080x100, r03r_ab_c4.log; with 256-thread
                               // workgroups the budget held ~95: 64 staged 132.15 ms, 16 133.31, none 132.98, r03h)
#endif
constexpr int kMaxLdsBlas = RT_LDS_BLAS_MAX;
// material and texture tables staged in LDS when both are this small (10 KB)
constexpr int kMaxLdsMaterials = 64;
// waves per CU the in-kernel reduction's ring is sized for (the launch clamps its grid to it): the
// spheres variant's 6 per SIMD, f64 and f32 (RT_BLOCK_SPHERES, RT_BLOCK_F32_SPHERES); 5 elsewhere
constexpr int kRingWavesSpheres = 24, kRingWavesOther = 20;

}  // namespace

// ---- shard geometry -----------------------------------------------------------------------------
int rows_in_shard(int height, int row_begin, int row_stride)
{
    if (height <= 0 || row_stride <= 0 || row_begin < 0 || row_begin >= height) return 0;
    return (height - row_begin + row_stride - 1) / row_stride;
}

// ceil(spp/16), at most 16 samples per work block (measured, pool schedule: C2 16 vs 32
// 99.4 / 100.4 ms, C4 16 vs 63 1565 / 1636 ms, C3 flat); a function of spp only, so the
// summation order (and the image) does not depend on launch geometry or sharding
int auto_chunk(int spp) { return std::min(16, std::max(1, (spp + 15) / 16)); }

int rows_in_band_shard(int height, int row_begin, int row_stride, int row_block)
{
    if (row_block <= 1) return rows_in_shard(height, row_begin, row_stride);
    if (height <= 0 || row_stride <= 0 || row_begin < 0 || (row_block & (row_block - 1)) || row_block > 64) return 0;
    const int bands = (height + row_block - 1) / row_block;
    const int mine = rows_in_shard(bands, row_begin, row_stride);
    if (!mine) return 0;
    const int last = row_begin + (mine - 1) * row_stride;   // its last band may be cut by the image
    return (mine - 1) * row_block + std::min(row_block, height - last * row_block);
}

int tiles_in_shard(int width, int height, int tile_begin, int tile_stride)
{
    if (width <= 0 || height <= 0) return 0;
    const long long tiles = (long long)((width + 7) / 8) * ((height + 7) / 8);
    if (tiles > 0x7fffffffLL) return 0;
    return rows_in_shard((int)tiles, tile_begin, tile_stride);
}

int row_block_of(const rt_render_params* p) { return p->row_block > 1 ? p->row_block : 1; }

Layout layout_of(const rt_render_params* p)
{
    if (p->tile_shard) {
        const int n = tiles_in_shard(p->width, p->height, p->row_begin, p->row_stride);
        return Layout{8 * n, n > 0 ? 8 : 0};
    }
    return Layout{p->width, rows_in_band_shard(p->height, p->row_begin, p->row_stride, row_block_of(p))};
}

bool bad_geometry(const rt_render_params* p)
{
    const int b = row_block_of(p);
    return p->width < 2 || p->height < 2 || p->row_stride < 1 || p->row_begin < 0 || p->spp_chunk < 0 ||
           (b & (b - 1)) || b > 64 || (long long)p->width * p->height > 0xffffffffLL ||
           (p->tile_shard != 0 && (p->tile_shard != 1 || b > 1));
}

// ---- inputs -------------------------------------------------------------------------------------
SceneFacts scene_facts(const rtl::Lowered& L, const rt_scene_soa& s)
{
    SceneFacts f;
    f.features = L.features;
    f.n_tlas_nodes = L.n_tlas_nodes;
    f.n_nodes = s.n_nodes;
    f.n_blas_bfs = L.n_blas_bfs;
    f.stack_entries = L.stack_entries;
    f.nested_stack_entries = L.blas_base + (L.blas_depth > 0 ? L.blas_depth + 1 : 0);
    f.stack16_ok = L.stack16_ok;
    f.n_materials = s.n_materials;
    f.n_textures = s.n_textures;
    f.pad_extent = L.pad_extent;
    f.has_moving = L.has_moving;
    f.time_lo = L.time_lo;
    f.time_hi = L.time_hi;
    return f;
}

double camera_magnitude(const rt_camera& cam)
{
    return std::sqrt(cam.origin[0] * cam.origin[0] + cam.origin[1] * cam.origin[1] + cam.origin[2] * cam.origin[2]) +
           std::fabs(cam.lens_radius) *
               (1.0 + std::sqrt(cam.u[0] * cam.u[0] + cam.u[1] * cam.u[1] + cam.u[2] * cam.u[2]) +
                std::sqrt(cam.v[0] * cam.v[0] + cam.v[1] * cam.v[1] + cam.v[2] * cam.v[2]));
}

// ---- the plan -------------------------------------------------------------------------------------
Plan plan(const SceneFacts& scene, const DeviceFacts& dev, const Options& opt, const Request& rq, const Retry& retry)
{
    Plan pl;
    const int chunk = rq.chunk, n_rows = rq.lay.rows;
    const long long n_px = (long long)n_rows * rq.lay.w;
    pl.px = (size_t)std::max<long long>(n_px, 1);

    pl.features = scene.features | opt.extra_features;
    pl.variant = rtk::variant_features(pl.features);
    const uint32_t variant = pl.variant;
    // conservative f32 slab tests need every ray origin within 2M of the origin (flatten.cpp):
    // hit points are inside the scene bounds; check the camera (+ lens) here
    pl.slab32 = opt.slab32 && scene.pad_extent > 0.0 && rq.cam_mag <= 2.0 * scene.pad_extent;
    pl.lds_stack = opt.lds_stack && scene.stack_entries <= kMaxLdsStack;
    pl.f32 = opt.precision == RT_PREC_F32;
    auto unsupported = [](const char* why) {
        Plan e;
        e.err = RT_ERR_UNSUPPORTED;
        e.err_msg = why;
        return e;
    };
    // a moving sphere's boxes bound it for ray times in the scene's [time_lo, time_hi] only
    // (flatten.cpp's box invariant), and camera rays carry times between time0 and time1:
    // outside, a node box could cull a sphere the exact test hits (negated: a NaN is refused too)
    if (scene.has_moving && !(std::min(rq.cam_time0, rq.cam_time1) >= scene.time_lo &&
                              std::max(rq.cam_time0, rq.cam_time1) <= scene.time_hi))
        return unsupported("the camera's time0 / time1 leave the time range the scene's boxes were built for "
                           "(rt_scene_soa.time_lo / time_hi; RT_BUILD_TIME0 / RT_BUILD_TIME1 before rt_world_flatten)");
    if (rq.moments && pl.f32) return unsupported("adaptive sampling in the f32 mode");
    if (pl.f32 && rq.count_work && variant != rtk::FEAT_SET_SPHERES && variant != rtk::FEAT_SET_FINAL)
        return unsupported("count_work in the f32 mode: the spheres and final-scene variants only");
    if (pl.f32) pl.slab32 = 1;   // statistical mode: f32 boxes whatever the camera
    // a scene with no BVH node (the Cornell scenes: one top-level leaf, instances over one
    // box) tests no slab: the f64-slab instantiation then, which holds no f32 ray terms
    // (rects + instances variant 125 vs 130 VGPRs: 4 vs 3 waves per SIMD)
    if (scene.n_nodes == 0 && !pl.f32) pl.slab32 = 0;
    const long long total = pl.total = rq.s_end - rq.s_begin;
    pl.n_chunks = (int)((total + chunk - 1) / chunk);
    const size_t px_bytes = pl.px_bytes = pl.px * 3 * sizeof(double);
    // one sample's records in the per-sample buffer: whole 8x8 tiles (trace_kernel.hpp, tiled_record)
    // (the f32 mode's records are f32: SampleTiles.f32_records; trace_pool writes them so)
    const size_t sample_bytes = pl.sample_bytes =
        rtk::tiled_pixels(rq.lay.w, n_rows) * 3 * (pl.f32 ? sizeof(float) : sizeof(double));
    // the TLAS in LDS (read-only, shared by the block) when it fits the per-block budget
    pl.n_lds_nodes = opt.lds_nodes ? std::min(scene.n_tlas_nodes, kMaxLdsNodes) : 0;
    // small material and texture tables in LDS too (the variants with rects or media)
    const bool stage = opt.lds_nodes && scene.n_materials <= kMaxLdsMaterials && scene.n_textures <= kMaxLdsMaterials &&
                       scene.n_materials > 0;
    pl.n_lds_materials = stage ? scene.n_materials : 0;
    pl.n_lds_textures = stage ? scene.n_textures : 0;
    // the kernel shape this launches (launch_shapes.hpp): its workgroup, launch bound and LDS layout
    const rtk::KernelShape& k = pl.shape = rtk::launch_shape(variant, pl.slab32 != 0, pl.lds_stack != 0, pl.f32 != 0, pl.n_lds_nodes,
                                                             scene.n_tlas_nodes, scene.stack16_ok != 0);
    const int bt = k.block_threads;
    const size_t wg_waves = (size_t)(bt / 64), cu_waves = 4 * (size_t)k.min_waves;   // 4 SIMDs per CU
    // the top levels of the BFS-ordered instance BLAS in LDS too (variants with nested walks),
    // as many as the LDS left over at the block count the rest of the layout allows
    pl.n_lds_blas = 0;
    if (scene.n_blas_bfs > 0 && opt.lds_nodes && (variant & rtk::FEAT_INST_BLAS) != 0) {
        const size_t base = rtk::lds_layout(k, pl.n_lds_nodes, 0, scene.stack_entries, pl.n_lds_materials, pl.n_lds_textures).total;
        // the CU's 160 KB shared by `blocks` workgroups, each allocation rounded up to the LDS
        // granule (taken as 1 KB; the occupancy API does not round: a layout it rated at 3
        // blocks per CU ran 2 and took 174 instead of 133 ms, r03g_ab_c4.log), and no more
        // workgroups than the variant's registers allow (final scene 4 waves per SIMD, the
        // all-features variant 3: 16 or 12 waves per CU)
        const size_t lds_cu = dev.lds_per_cu, granule = 1024;
        const size_t wave_blocks = std::max<size_t>(1, cu_waves / wg_waves);
        const size_t blocks = std::max<size_t>(1, std::min(wave_blocks,
            lds_cu / (((std::max<size_t>(base, 1) + granule - 1) / granule) * granule)));
        const size_t budget = std::min(lds_cu / blocks, dev.lds_per_block) / granule * granule;
        const size_t spare = budget > base ? budget - base : 0;
        pl.n_lds_blas = (int32_t)std::min<size_t>({(size_t)scene.n_blas_bfs, spare / rtk::kBvhNodeBytes, (size_t)kMaxLdsBlas});
    }
    // work blocks of one tile: 16-sample chunks, per-sample pool one chunk per block, item pool
    // two (C2 kernel ms, pool 1/2/4 chunks: 99.8/100.2/103.2; items 1/2/4: 106.8/104.1/105.0;
    // profiles/r02f_*, r02g_*)
    pl.block_chunks = opt.block_chunks > 0 ? opt.block_chunks : 2;
    // Schedule and buffer batches, from the context's trace-output bound (sample_buf_cap). The
    // bound is sized from the free HBM when the context is created; if the device has less by
    // now (another context, torch or RCCL allocated since), the allocation fails and the
    // bound is halved until it fits (shrink): more batches (or the item pool), the same image.
    // per-sample pool blocks: the chunk's 16 samples per tile while that leaves >= 160 k blocks
    // (~40 per resident wave), else halved down to 4: a small shard's last blocks would
    // otherwise leave waves idle (C2 rows of 1 of 8 GPUs: 16 / 8 / 4 samples 14.06 / 13.70 /
    // 13.57 ms; the whole frame 99.9 / 100.0 / 101.4; scripts/shard_coherence.py, r02p)
    if (opt.block_samples > 0) {
        pl.block_samples = opt.block_samples;
    } else {
        const long long tiles = (long long)((rq.lay.w + 7) / 8) * ((n_rows + 7) / 8);
        int bs = chunk;
        while (bs > 4 && tiles * ((total + bs - 1) / bs) < 160000) bs = (bs + 1) / 2;
        pl.block_samples = bs;
    }
    // the pool's in-kernel reduction needs blocks of exactly one chunk (a block's sum is the
    // chunk's) and batches on chunk boundaries; its ring: kPoolRing blocks for each wave of the
    // persistent grid (kRingWaves* per CU)
    const bool ring_ok = retry.ring_allowed && opt.ring && pl.block_samples == chunk &&
                         chunk <= (int)(rtk::kRingSlot / 64) && rq.s_end <= (int)rtk::kRingSampleMask;
    const int ring_waves = dev.n_cus * (variant == rtk::FEAT_SET_SPHERES ? kRingWavesSpheres : kRingWavesOther);
    const size_t ring_bytes = (size_t)ring_waves * rtk::kRingWaveDoubles * sizeof(double);
    // halved on an out-of-memory retry for this render only: the context's bound stays, so a
    // later render on it uses the memory freed since
    const size_t buf_cap = retry.buf_cap;

    // AUTO: the per-sample pool when its per-sample radiance is at most 4 times the bound,
    // else the item pool, whose partials take 1/chunk of those bytes (C5's 1.6 TB: one launch).
    // Round 2, pool vs items: C2 101.6 vs 106.7 ms per frame, C4 1492 vs 1571 (r02d_*, r02e_*);
    // round 4: C2 74.75 vs 76.06, C4 1018.5 vs 1074.7; C5 in 25 overlapped pool batches of
    // 64 GB halves 10,578 ms vs the item pool 10,649 in 64 batches at a 4 GB bound (r04f_*)
    // AUTO, measured per variant (round 5, profiles/r05x_*, r05w_*, r05y_*): the Cornell box takes
    // the item pool (C3 800x800x1000: items 204.5 ms, per-sample buffer 209.9, ring 215.0); the
    // others the per-sample pool — its buffer while that fits the bound in one batch (C1: 2.03 ms,
    // ring 2.06), else the ring (C2: 74.0 vs 74.7 unbounded; C4 x256: 267.3, items 291.8) — and
    // the item pool only when neither fits
    // (the media variant, Cornell smoke 600x600x200: items 31.72 ms, per-sample buffer 30.28: pool)
    const bool cornell = variant == rtk::FEAT_SET_RECTINST;
    const bool fits_one = (size_t)total * sample_bytes <= buf_cap;
    pl.schedule = rq.moments                     ? RT_SCHED_POOL
                  : opt.schedule != RT_SCHED_AUTO ? opt.schedule
                  : cornell && !pl.f32 ? RT_SCHED_ITEMS
                  : (ring_ok || (size_t)total * sample_bytes <= 4 * buf_cap ? RT_SCHED_POOL : RT_SCHED_ITEMS);
    // POOL with the in-kernel reduction: chunk partials like ITEMS (the ring takes its share of
    // the bound first, the partials at least one chunk)
    pl.ring = pl.schedule == RT_SCHED_POOL && ring_ok && (opt.ring == 2 || !fits_one) && !rq.moments;
    // overlapped batches trace two launches at once, a ring each: a render that does not fit
    // one batch beside one ring budgets two
    size_t out_cap = buf_cap;
    if (pl.ring) {
        const size_t all = (size_t)pl.n_chunks * px_bytes;
        const int rings = opt.overlap && all + ring_bytes > buf_cap ? 2 : 1;
        out_cap = std::max(buf_cap > rings * ring_bytes ? buf_cap - rings * ring_bytes : 0, px_bytes);
    }
    // Buffer batches: the trace output is bounded by sample_buf_cap. Per-sample pool: samples x
    // pixels x 24 B; chunk and item schedules: chunks x pixels x 24 B, batches on chunk
    // boundaries (relative to s_begin), so the partials add in one-launch order. A render that
    // does not fit in one batch takes two buffers of half the bound: batch k traces into half
    // k & 1 on stream tstream[k & 1] while the caller's stream reduces batch k - 1, so the
    // next trace fills the CUs its predecessor's last waves leave (no tail per batch).
    pl.per_sample = pl.schedule == RT_SCHED_POOL && !pl.ring;
    // Wave-wide sample starts (launch_shapes.hpp, RT_STAGE_SEEDS): the f64 spheres variant's
    // 16-bit-stack per-sample pool kernels, buffer and ring forms, keep one 32 B slot per lane in LDS
    // after the stack — while that costs the variant no resident workgroup (6 waves per SIMD: 24
    // per CU; each allocation rounded to the 1 KB granule as for the staged BLAS above). The random
    // scene: 22.2 KB of node records + 19.5 KB of stack + 24 KB = 66 KB, two 768-thread workgroups in
    // 160 KB as before; a scene whose stack leaves no room keeps the per-lane sample starts.
    if (RT_STAGE_SEEDS && k.s16 && !pl.f32 && pl.schedule == RT_SCHED_POOL) {
        const size_t granule = 1024, stage = rtk::seed_stage_bytes_of(bt);
        const size_t base = rtk::lds_seeds_offset(rtk::lds_layout(k, pl.n_lds_nodes, 0, scene.stack_entries, 0, 0).total);
        auto resident = [&](size_t bytes) {
            const size_t alloc = (std::max<size_t>(bytes, 1) + granule - 1) / granule * granule;
            return alloc > dev.lds_per_block ? (size_t)0 : std::min(std::max<size_t>(1, cu_waves / wg_waves), dev.lds_per_cu / alloc);
        };
        if (resident(base + stage) > 0 && resident(base + stage) == resident(base)) pl.seed_stage_bytes = stage;
    }
    const size_t unit = pl.per_sample ? sample_bytes : px_bytes;
    long long fit = (long long)std::max<size_t>(1, out_cap / unit);
    pl.batch = std::min<long long>(total, pl.per_sample ? fit : fit * chunk);
    // (only with 256-thread workgroups: a batch's launch of the large-workgroup variants —
    // the spheres variant's 768 threads, the final scene's 1024 — takes a CU only when a whole
    // workgroup of its predecessor has left, and the two persistent grids then contend instead:
    // C5 4096x4096x4096 overlapped 11,471 ms per frame, in order 10,474, profiles/r06zz_c5_*)
    pl.overlap = opt.overlap && bt <= 256 && pl.batch < total && pl.schedule != RT_SCHED_CHUNKS;
    if (pl.overlap) {
        fit = (long long)std::max<size_t>(1, out_cap / 2 / unit);
        pl.batch = std::min<long long>(total, pl.per_sample ? fit : fit * chunk);
    }
    pl.n_batches = (int)((total + pl.batch - 1) / pl.batch);
    // (an adaptive pass keeps its sums and the open chunk in the call's frame-layout accumulators)
    if (pl.per_sample && !rq.moments && (pl.n_batches > 1 || rq.acc_sink)) {  // [open chunk sums | running total (no acc sink)]
        pl.open_chunk = true;
        pl.own_total = !rq.acc_sink;
        pl.acc_bytes = 2 * px_bytes;
    } else if (!pl.per_sample && pl.n_batches > 1 && !rq.acc_sink) {  // running total of the chunk partials
        pl.own_total = true;
        pl.acc_bytes = px_bytes;
    }
    const int max_chunks = (int)((pl.batch + chunk - 1) / chunk);
    pl.half_bytes = pl.per_sample ? (size_t)pl.batch * sample_bytes : (size_t)max_chunks * px_bytes;
    pl.partial_bytes = pl.overlap ? 2 * pl.half_bytes : pl.half_bytes;
    pl.ring_waves = pl.ring ? ring_waves : 0;
    pl.ring_one_bytes = pl.ring ? ring_bytes : 0;
    pl.ring_bytes = (pl.overlap ? 2 : 1) * pl.ring_one_bytes;   // one ring per trace stream
    pl.trace_buf_bytes = pl.partial_bytes + pl.ring_bytes;
    return pl;
}

bool shrink(const Plan& pl, Retry& retry)
{
    if (retry.buf_cap <= ((size_t)1 << 20) || pl.partial_bytes <= (pl.per_sample ? pl.sample_bytes : pl.px_bytes))
        return false;
    retry.buf_cap = std::max<size_t>(retry.buf_cap / 2, (size_t)1 << 20);
    return true;
}

}  // namespace rtp
