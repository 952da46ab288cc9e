// trace_device.hpp — the MI355X megakernel for the reference's per-(pixel, sample)
// hot path: Camera::get_ray (camera.rs:58-66) + ray_color (main.rs:19-38) and
// everything below it (hittable.rs, material.rs, texture.rs, perlin.rs), in f64
// like the reference (math.rs:13-17).
//
// Execution model:
//   * work unit = one (pixel, sample) path; work block = one 8x8 pixel tile x one chunk
//     of spp_chunk samples (a function of spp only);
//   * trace_pool (default): persistent waves take blocks from a device counter, and a
//     lane whose path ended takes the block's next unit in the same bounce-loop
//     iteration (ballot + mbcnt), so lanes do not idle until the last blocks run out;
//     each sample's radiance goes to its slot of a per-sample buffer (tiled) and
//     reduce_samples_tiled sums every pixel's samples in sample order, chunk by chunk — the
//     image does not depend on which lane computed a sample, on the launch geometry or
//     on how rows are sharded over GPUs; trace_chunks (the first schedule, kept for A/B)
//     gives a lane one pixel's chunk and adds the same partial sums;
//   * the depth-50 recursion is an iterative bounce loop; traversal carries only
//     (t, primitive slot); the HitRecord (hittable.rs:6-27) is built once per cast;
//   * TLAS nodes and the traversal stack in LDS, conservative f32 slab tests, f64
//     primitive tests; materials share their expensive steps so a wave holding several
//     kinds runs each step once;
//   * RNG: per (pixel, sample) a Philox4x32-10 block seeds a xoshiro128++ path stream
//     (rt_numerics.h); the medium's in-hit draw is keyed by (pixel, sample, bounce, medium id).
// Built with -ffp-contract=off: bit-for-bit the operation order of the reference.
//
// The code, by layer; each header includes the ones below it. The order is part of the build: a
// code object holds its kernels in the order they are first named (scripts/device_code_hashes.py).
#pragma once
#include "trace_types.hpp"    // rays, hit records, counters, Cfg, the stack, div_rcp, r_*, finish_ray
#include "trace_prims.hpp"    // sphere, rect and box tests, slab tests, simple_t / simple_finish
#include "trace_walk.hpp"     // nodes in LDS, traverse, instances, media, finish_hit, trace_world
#include "trace_shade.hpp"    // Perlin, textures, the path stream, the camera, stage_lds, shade_*
#include "trace_grid.hpp"     // image_row, image_xy, lane_work, min_waves
#include "trace_chunks.hpp"   // the chunk schedule: trace_chunks
#include "trace_pool.hpp"     // the pool schedules: the ring, the deal order, staged seeds, trace_pool
