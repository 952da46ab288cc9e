// launch_plan.hpp — what a render of one sample range launches, decided from a few dozen
// integers: the kernel configuration (f32 or f64 slabs, where the stack lives, what is staged in
// LDS), the schedule, the buffer batches and the memory they need. Pure arithmetic, no HIP and no
// context: abi.cpp's run_range allocates and enqueues what plan() returns; tests/plan_dump.cpp
// runs it on a CPU. The shard geometry of rt_render_params lives here too.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rt/rt_abi.h"
#include "launch_shapes.hpp"
#include "scene_lower.hpp"

namespace rtp {

// ---- shard geometry (the extern "C" rt_rows_in_shard, ... forward to these) --------------------
int rows_in_shard(int height, int row_begin, int row_stride);
int rows_in_band_shard(int height, int row_begin, int row_stride, int row_block);
int tiles_in_shard(int width, int height, int tile_begin, int tile_stride);
int row_block_of(const rt_render_params* p);
// The shard's output layout (the kernel's pixel grid): its rows of the image, or (tile_shard)
// its 8x8 tiles side by side in one 8-row slab
struct Layout {
    int w, rows;
};
Layout layout_of(const rt_render_params* p);
bool bad_geometry(const rt_render_params* p);
int auto_chunk(int spp);

// ---- the plan's inputs --------------------------------------------------------------------------
struct SceneFacts {   // what the context keeps of an uploaded scene
    uint32_t features = 4095;   // rtk::FEAT_* of the scene (FEAT_ALL until one is uploaded)
    int n_tlas_nodes = 0;
    int n_nodes = 0;            // BVH nodes of the scene (TLAS + BLASes)
    int n_blas_bfs = 0, stack_entries = 0, stack16_ok = 0;   // rtl::Lowered's fields of these names
    // the entries of a walk that nests every BLAS walk in the top-level one, deferring none
    // (stack_entries may count on the trace kernels' deferred first instance: scene_lower.cpp);
    // rt_trace_rays' launches are planned and laid out with it
    int nested_stack_entries = 0;
    int n_materials = 0, n_textures = 0;
    double pad_extent = 0.0;
    // the scene holds a moving sphere, whose boxes bound it for ray times in [time_lo, time_hi]
    // (rtl::Lowered's fields of these names; rt_scene_soa.time_lo / time_hi)
    int has_moving = 0;
    double time_lo = 0.0, time_hi = 1.0;
};
SceneFacts scene_facts(const rtl::Lowered& L, const rt_scene_soa& s);

struct DeviceFacts {   // read when the context is created
    int n_cus = 256;
    size_t lds_per_cu = 160 * 1024;     // the device's LDS per CU and per workgroup
    size_t lds_per_block = 160 * 1024;
};

struct Options {   // the context's switches
    int slab32 = 1, lds_stack = 1, lds_nodes = 1;   // rt_ctx_set_variant
    int schedule = RT_SCHED_AUTO;                   // rt_ctx_set_schedule
    int precision = RT_PREC_F64;                    // rt_ctx_set_precision
    int ring = 1;                                   // RT_OPT_POOL_RING: POOL reduces finished blocks in the kernel (0 never,
                                                    // 1 when its per-sample buffer would not fit the bound, 2 always)
    int overlap = 1;                                // RT_OPT_BATCH_OVERLAP
    int block_chunks = 0;                           // RT_OPT_BLOCK_CHUNKS: chunks per item-pool work block (0: auto)
    int block_samples = 0;                          // RT_OPT_BLOCK_SAMPLES: samples per per-sample-pool work block (0: auto)
    uint32_t extra_features = 0;                    // RT_OPT_EXTRA_FEATURES: a larger kernel variant than the scene needs (tests)
};

struct Request {
    Layout lay{0, 0};           // layout_of(params)
    int s_begin = 0, s_end = 0, chunk = 1;   // samples [s_begin, s_end) in chunks of `chunk`
    bool count_work = false;
    bool acc_sink = false;      // the sums are added to a caller's accumulator (rt_accum_add)
    bool moments = false;       // an rt_render_adaptive pass: the moments sink
    double cam_mag = 0.0;       // camera_magnitude(camera)
    double cam_time0 = 0.0, cam_time1 = 1.0;   // the camera's shutter: every ray time lies between them
};
// how far from the origin a camera ray can start (the camera and its lens): the slab32 test
double camera_magnitude(const rt_camera& cam);

// what run_range's out-of-memory loop varies between attempts
struct Retry {
    size_t buf_cap = 0;         // the trace-output bound of this attempt (the context's at first)
    bool ring_allowed = true;   // false once the ring itself did not fit
};

// ---- the plan -------------------------------------------------------------------------------------
struct Plan {
    int err = RT_OK;            // RT_ERR_UNSUPPORTED (and why) for the two f32 cases no kernel serves and for a
    const char* err_msg = "";   // camera shutter outside the scene's time range: nothing below is set then
    // the launch options
    uint32_t features = 0;      // scene features | extra features
    uint32_t variant = 0;       // rtk::variant_features of them
    int slab32 = 0, lds_stack = 0, f32 = 0;
    int schedule = 0;           // RT_SCHED_*, AUTO resolved
    rtk::KernelShape shape{};   // the kernel instantiation those options and the staged TLAS launch (launch_shapes.hpp)
    // staged in LDS (SceneDev's fields of these names)
    int n_lds_nodes = 0, n_lds_materials = 0, n_lds_textures = 0, n_lds_blas = 0;
    // LDS bytes per workgroup of the wave-wide sample starts (SceneDev.seed_stage_bytes; launch_shapes.hpp
    // RT_STAGE_SEEDS): 32 B x 64 x the workgroup's waves on the kernels that stage, 0 on all others
    size_t seed_stage_bytes = 0;
    // work blocks, the in-kernel reduction
    int block_chunks = 0, block_samples = 0;
    bool ring = false;
    int ring_waves = 0;         // waves the ring holds (0: no ring)
    bool per_sample = false;    // the trace output is per-sample records (else chunk partials)
    // buffer batches
    long long total = 0;        // samples of the range
    int n_chunks = 0;           //   and its chunks
    long long batch = 0;        // samples per batch (the last one may be shorter)
    int n_batches = 0;
    bool overlap = false;       // batches alternate between two buffer halves and two trace streams
    // memory, each size computed once
    size_t px = 1;              // pixels of the shard (at least 1)
    size_t px_bytes = 0;        // one f64 RGB sum per pixel
    size_t sample_bytes = 0;    // one sample's records in the per-sample buffer
    size_t half_bytes = 0;      // one buffer half: the largest batch's trace output
    size_t partial_bytes = 0;   // the halves together
    size_t ring_one_bytes = 0;  // one trace stream's ring (0: no ring)
    size_t ring_bytes = 0;      // the rings together
    size_t trace_buf_bytes = 0; // partial_bytes + ring_bytes
    // accumulators beside the sink: the open chunk's sums carried across per-sample batches, and a
    // running total of our own (when batches add up and the sink is not an accumulator itself)
    bool open_chunk = false, own_total = false;
    size_t acc_bytes = 0;       // their allocation ([open chunk | running total], or the total alone)
};

Plan plan(const SceneFacts& scene, const DeviceFacts& dev, const Options& opt, const Request& rq, const Retry& retry);

// After an attempt whose trace-output buffer did not fit the device: halves the bound (at least
// 1 MiB) for the next one; false when this attempt was already the smallest batch.
bool shrink(const Plan& pl, Retry& retry);

}  // namespace rtp
