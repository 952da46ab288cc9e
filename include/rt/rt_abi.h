/*
 * rt_abi.h — the drop-in boundary: a C ABI (plain pointers and sizes) over the
 * MI355X path tracer. Every entry point returns RT_OK (0) or a negative RT_ERR_*
 * code; nothing aborts and no C++ exception crosses it.
 *
 * What it replaces in the reference (paths relative to /root/reference/src):
 *
 *   rt_render                 the per-(pixel, sample) driver loop main.rs:497-551
 *                             = Camera::get_ray (camera.rs:58-66) followed by
 *                             ray_color (main.rs:19-38) per sample, summed per
 *                             pixel and divided by spp (math.rs:119-126)
 *   rt_camera_new             Camera::new (camera.rs:18-56)
 *   rt_world_*                World + register_material (main.rs:40-50) and the
 *                             Hittable / Material / Texture constructors
 *                             (hittable.rs:77-207, material.rs:6-12, texture.rs:4-22,
 *                             perlin.rs:13-30)
 *   rt_world_build_scene      the scene builders main.rs:52-289
 *   rt_scene_preset           the per-scene camera/background table main.rs:314-464
 *   rt_world_flatten          (new) lowers the Hittable tree to rt_scene_soa
 *   rt_ctx_upload_*           (new) copies the SoA tables into HBM
 *   rt_write_ppm              write_color + the P3 writer (math.rs:119-132,
 *                             main.rs:472, 591-596)
 *   rt_accum_* /              the per-thread partial sums, their merge into the shared
 *   rt_render_progressive     buffer and the progress channel (main.rs:504-582), as
 *                             resumable sample batches with a progress callback
 *   rt_comm_* /               the partition of one frame over workers (main.rs:497-551)
 *   rt_render_gather          and the merge of their buffers (main.rs:542-547), over GPUs:
 *                             8x8 tile shards, one RCCL gather to rank 0, a reorder kernel
 *   rt_render_adaptive        (new) the same driver loop with the per-pixel sample count
 *                             (main.rs:516) decided per 8x8 tile from the estimate's noise
 *   rt_denoise                (new) a post-filter over the adaptive frame and its noise map; the
 *                             reference has no filter
 *   rt_render_features        (new) the first hit of the same primary rays (camera.rs:58-66) as
 *                             albedo, normal and depth buffers; the reference writes none
 *   rt_denoise_guided         (new) rt_denoise with those buffers in its weights
 *   rt_denoise_atrous         (new) a second post-filter: an edge-stopping a-trous wavelet over the
 *                             same inputs, which also hands back the noise left in its result
 *   rt_render_adaptive_halves (new) rt_render_adaptive that also hands back the means of the even and
 *                             of the odd samples
 *   rt_denoise_cross          (new) rt_denoise over two half frames, each filtered with the other's
 *                             weights, with the error left read off their difference
 *   rt_denoise_pyramid        (new) rt_denoise_guided run at several scales of the frame, the coarse
 *                             scales supplying the low frequencies its window cannot see
 *   rt_adaptive_state_*       (new) rt_render_adaptive's accumulators kept between calls: the frame
 *                             tightened, previewed, checkpointed, or steered by a caller's error map
 *   rt_trace_rays             (new) hit_hittables (hittable.rs:43-55) for rays the caller states:
 *                             the closest hit's record, or whether anything is hit at all
 *   rt_camera_rays            (new) Camera::get_ray (camera.rs:58-66) for every pixel of a frame,
 *                             written out as the rays rt_render shoots
 *
 * Threading: a context is bound to one device and is used by one host thread at
 * a time. Worlds are plain host objects.
 */
#ifndef RT_ABI_H
#define RT_ABI_H

#include <stddef.h>
#include <stdint.h>

#include "rt_scene.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 6   /* v6: RT_OPT_COMM_DIRECT */

enum {
    RT_OK = 0,
    RT_ERR_INVALID = -1,      /* bad argument / handle */
    RT_ERR_HIP = -2,          /* a HIP runtime call failed (see rt_last_error) */
    RT_ERR_UNSUPPORTED = -3,  /* a Hittable nesting the flattener does not lower */
    RT_ERR_OOM = -4,
    RT_ERR_NO_DEVICE = -5,
    RT_ERR_NO_SCENE = -6,     /* render before upload */
    RT_ERR_COMM = -7,         /* an RCCL call failed, or RCCL could not be loaded (see rt_last_error) */
    RT_ERR_PEER = -8          /* a collective call failed on another rank; this rank's state is consistent */
};

typedef struct rt_ctx rt_ctx;
typedef struct rt_world rt_world;

int rt_abi_version(void);
/* Text of the last error on this thread ("" if none). */
const char* rt_last_error(void);
/* Build identity of the loaded library: the source hash it was compiled from (16 hex digits
 * of sha256 over csrc/, include/rt/ and the compile flags: __graft_entry__.source_hash()),
 * "unknown" for a build without one. Profiles and PMC records are keyed by it, so a caller can
 * check that the library it times is the build its counters describe. */
const char* rt_build_info(void);

/* ---- device context --------------------------------------------------------- */
int rt_device_count(int* count);
int rt_ctx_create(int device, rt_ctx** out);
void rt_ctx_destroy(rt_ctx* ctx);

/* ---- host scene model (the reference's World / Hittable surface) --------------- */
/* A world owns a seeded construction stream (Philox, rt_numerics.h) that replaces
 * thread_rng() during scene building (random_double in main.rs:191,233,256-268,
 * perlin.rs:16-22,123-124, hittable.rs:82). */
int rt_world_create(uint64_t scene_seed, rt_world** out);
void rt_world_destroy(rt_world* w);

/* Textures (texture.rs:4-22) -> texture id >= 0.
 * Where the values are the reference's (texture.rs:30-75). The sine under the checker and the noise
 * (rt_sin, rt_numerics.h) is accurate for |x| < 2^20 * pi / 2 = 1.647e6, and Perlin's lattice index is
 * an i32 of 64 p at the seventh octave. So at a point p
 *   - the checker texture is the reference's while |10 * p_i| < 2^20 * pi / 2 on each axis, that is
 *     |p_i| < 1.647e5;
 *   - the noise texture is the reference's while |scale * p.z| < 2^20 * pi / 2 and every |p_i| < 2^25
 *     (from 2^25 the reference itself saturates the cast and then overflows `i + 1`);
 *   - the image texture has no such limit.
 * Beyond those limits the values are deterministic (a function of the scene and p alone, the same on
 * the host and on the device, in renders, feature buffers and rt_trace_rays' albedo) but not the
 * reference's: a checker cell may take the other colour from |10 p_i| of about 1.6e7, and a noise
 * value may leave [0, 1] from |scale * p.z| of about 2^40 and is inf or NaN from about 2^120.
 * tests/test_texture_reference.py and tests/test_gpu_textures.py hold the textures to an independent
 * high-precision evaluation inside the limits, and the device to the host's bits outside them. The
 * built-in scenes stay far inside (|p| <= 1000, |scale * p.z| <= 4000). */
int rt_world_texture_solid(rt_world* w, double r, double g, double b, int* tex_out);
int rt_world_texture_checker(rt_world* w, const double even[3], const double odd[3], int* tex_out);
/* Perlin::new() draws from the world's stream (perlin.rs:13-30). */
int rt_world_texture_noise(rt_world* w, double scale, int* tex_out);
/* RGB8 texels as stb_image returns them; the world copies them. */
int rt_world_texture_image(rt_world* w, const uint8_t* rgb, int width, int height, int* tex_out);

/* Materials (material.rs:6-12) -> 1-based MaterialHandle (main.rs:46-49). */
int rt_world_material_lambertian(rt_world* w, int tex, int* handle_out);
int rt_world_material_metal(rt_world* w, const double albedo[3], double fuzz, int* handle_out);
int rt_world_material_dielectric(rt_world* w, double ir, int* handle_out);
int rt_world_material_diffuse_light(rt_world* w, int tex, int* handle_out);
int rt_world_material_isotropic(rt_world* w, int tex, int* handle_out);

/* Hittables (hittable.rs:30-41, constructors :77-207) -> hittable id >= 0.
 * The constructors take every value the reference's take, and a world built from them either
 * renders what the reference computes for it or is refused with a message before any launch
 * (the context stays usable):
 *   a radius < 0 (the hollow-glass idiom)  accepted: hit by |radius|, normals divided by radius
 *   a moving sphere's shutter (t0, t1)     t0 == t1 or a non-finite value: RT_ERR_INVALID (the centre
 *                                          divides by t1 - t0); otherwise accepted, also t0 > t1 and
 *                                          shutters beside [0, 1]; its centre extrapolates to any
 *                                          ray time, and the boxes cover the build's time range
 *                                          (RT_BUILD_TIME0 / _TIME1, default [0, 1]); rt_render
 *                                          and the other passes refuse a camera whose time0 / time1
 *                                          leave that range (RT_ERR_UNSUPPORTED) when the scene
 *                                          holds a moving sphere
 *   rt_world_bvh over a child whose reference bounding box does not bound it (a sphere of
 *   radius < 0, or a moving sphere whose own shutter does not cover the build's time range,
 *   not wrapped in a rotate_y, whose box is a hull of corners): the reference culls by that
 *   box, so its image depends on its hierarchy; rt_world_flatten / rt_ctx_upload_world refuse
 *   the world with RT_ERR_UNSUPPORTED, naming the node and the child, in every accel mode
 *   chains of more than 4 translate / rotate_y, and a medium boundary holding instances or
 *   media: RT_ERR_UNSUPPORTED at flatten, as before. */
int rt_world_sphere(rt_world* w, int mat, const double center[3], double radius, int* id_out);
int rt_world_moving_sphere(rt_world* w, int mat, const double c0[3], const double c1[3], double t0, double t1,
                           double radius, int* id_out);
/* axis: 0 XYRect (k on z), 1 XZRect (k on y), 2 YZRect (k on x). */
int rt_world_rect(rt_world* w, int axis, int mat, double a0, double a1, double b0, double b1, double k,
                  int* id_out);
int rt_world_box(rt_world* w, const double mn[3], const double mx[3], int mat, int* id_out);
int rt_world_translate(rt_world* w, int child, const double offset[3], int* id_out);
int rt_world_rotate_y(rt_world* w, int child, double angle_degrees, int* id_out);
int rt_world_constant_medium(rt_world* w, int boundary, double density, int phase_mat, int* id_out);
/* new_bvh_node(list, 0, n, t0, t1): random axis + median split, draws from the stream. */
int rt_world_bvh(rt_world* w, const int* ids, int n, double t0, double t1, int* id_out);
/* world.hittables.push(id) */
int rt_world_push(rt_world* w, int id);

/* Built-in scene builders, ids as the reference's match arms (main.rs:314-464):
 * 0 random, 1 two_spheres, 2 two_perlin, 3 earth, 4 simple_light, 5 cornell,
 * 6 cornell_smoke, 7 final. Scenes 3 and 7 need the earth texture (RGB8). */
int rt_world_build_scene(rt_world* w, int scene_id, const uint8_t* image_rgb, int image_w, int image_h);

typedef struct rt_world_info {
    int32_t n_hittables;     /* top-level list length */
    int32_t n_materials;
    int32_t n_leaf_prims;    /* leaves reachable from the list */
    int32_t n_media;
    double checksum;         /* same probe as the oracle's orc_scene_info */
} rt_world_info;
int rt_world_info_get(const rt_world* w, rt_world_info* out);

/* ---- camera ----------------------------------------------------------------------- */
int rt_camera_new(const double look_from[3], const double look_at[3], const double vup[3], double vfov,
                  double aspect_ratio, double aperture, double focus_dist, double time0, double time1,
                  rt_camera* out);

typedef struct rt_scene_preset {
    double look_from[3], look_at[3], background[3];
    double vfov, aperture, focus_dist, time0, time1;
    int32_t default_width, default_spp;   /* the reference's own image_width / samples_per_pixel */
    double default_aspect;
} rt_scene_preset;
int rt_scene_preset_get(int scene_id, rt_scene_preset* out);
/* Preset camera for an explicit width x height (aspect = width/height). */
int rt_scene_camera(int scene_id, int width, int height, rt_camera* cam_out, double background_out[3]);

/* ---- lowering + upload ---------------------------------------------------------------- */
/* SAH builder options of this world's rt_world_flatten (the tree changes, the image does not):
 * value < 0 (or 0 for the sizes and the cost) restores the default. Tuning knobs for A/B runs
 * (scripts/ab_variants.py --bvh); the defaults are DESIGN.md §2's. */
enum {
    RT_BUILD_C_ISECT = 1,          /* primitive-test cost relative to a node visit (default 1) */
    RT_BUILD_MAX_LEAF = 2,         /* largest leaf the cost model may pick (8) */
    RT_BUILD_FORCE_LEAF = 3,       /* a set this small is always one leaf (2) */
    RT_BUILD_ROOT_LEAF = 4,        /* a whole BVH of at most this many items is one leaf (8) */
    RT_BUILD_SPLIT_BOX_PAIRS = 5,  /* pairs holding a Box, a medium or a BLAS instance split by cost (1) */
    RT_BUILD_SPLIT_BLAS_PAIRS = 6, /* pairs inside instance BLASes split by cost (1) */
    /* not tuning knobs: the ray times [min, max] of the two the node boxes are built for (0 and 1),
     * any finite value taken as it is; set them to the shutter of the camera the world will be
     * rendered with when that is not within [0, 1] (rt_scene_soa.time_lo / time_hi) */
    RT_BUILD_TIME0 = 7,
    RT_BUILD_TIME1 = 8
};
int rt_world_set_build_option(rt_world* w, int key, double value);
/* Flattens the world into SoA tables owned by the world (valid until the next
 * flatten or rt_world_destroy). accel: RT_ACCEL_SAH / _LINEAR / _MEDIAN (rt_scene.h). */
int rt_world_flatten(rt_world* w, int accel, const rt_scene_soa** soa_out);
/* Checks a (possibly foreign) SoA the way rt_ctx_upload_soa does before copying it: every
 * index in range, no cycle in the node graph, and the traversal stack each walk needs
 * (computed from the tables; the soa's tlas_depth / blas_depth fields are not trusted).
 * Host only, no device needed. Depth outputs may be NULL. */
int rt_scene_validate(const rt_scene_soa* soa, int32_t* tlas_depth, int32_t* blas_depth);
int rt_ctx_upload_soa(rt_ctx* ctx, const rt_scene_soa* soa);
int rt_ctx_upload_world(rt_ctx* ctx, rt_world* w, int accel);

/* ---- render ----------------------------------------------------------------------------- */
enum { RT_OUT_F32 = 0, RT_OUT_F64 = 1 };

typedef struct rt_render_params {
    int32_t width, height;       /* full image */
    int32_t spp, max_depth;
    int32_t spp_chunk;           /* samples a lane sums before its partial is written; 0 = auto */
    int32_t row_begin, row_stride; /* rows rendered: y = row_begin + k*row_stride < height (y = 0 bottom) */
    int32_t out_format;          /* RT_OUT_F32 / RT_OUT_F64 */
    int32_t out_on_device;       /* 0: out is host memory (copied back); 1: out is a device pointer */
    int32_t count_work;          /* 1: also count casts / node visits / prim tests (slower) */
    double background[3];
    uint64_t render_seed;
    void* stream;                /* hipStream_t to launch on (NULL = the context's stream) */
    int32_t row_block;           /* 0 / 1: rows as above. B > 1 (a power of two <= 64): the image is cut
                                    into bands of B rows and the shard is bands j = row_begin +
                                    m*row_stride (rows jB .. jB+B-1 < height): row-band interleave, so
                                    a multi-GPU shard keeps 8x8 work tiles contiguous in the image */
    int32_t tile_shard;          /* 0: rows as above. 1 (row_block 0 / 1): the shard is the 8x8 pixel tiles
                                    t = row_begin + m*row_stride of the frame's tile grid (ceil(width/8)
                                    tiles per tile row, t = ty*ceil(width/8) + tx), written side by side
                                    as one 8-row slab: out row k holds rows 8*ty + k of the shard's
                                    tiles, tile m in columns 8m .. 8m+7 (rt_tiles_in_shard tiles; the
                                    pixels of an edge tile past the image are rendered and meaningless).
                                    Every shard is whole 8x8 tiles, so a multi-GPU shard keeps the
                                    kernel's work tiles compact in the image at any GPU count. With a
                                    tile order set on the context (rt_ctx_set_tile_order), t is a
                                    position in that order: the shard's tile m is order[row_begin +
                                    m*row_stride]. */
} rt_render_params;

/* Renders the selected rows (or tiles) into out (rows_local x width x 3, row k = the k-th
 * selected row; tile shards: 8 x (8 * tiles_local) x 3) as the per-pixel mean radiance
 * sum * (1/spp). Synchronous unless out_on_device is set, in which case the work is only
 * enqueued on `stream`. */
int rt_render(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, void* out);

/* Rows rendered for (height, row_begin, row_stride). */
int rt_rows_in_shard(int height, int row_begin, int row_stride);
/* Rows rendered for (height, row_begin, row_stride, row_block) (rt_render_params.row_block). */
int rt_rows_in_band_shard(int height, int row_begin, int row_stride, int row_block);
/* 8x8 tiles rendered for (width, height, row_begin, row_stride) with tile_shard = 1. */
int rt_tiles_in_shard(int width, int height, int tile_begin, int tile_stride);

typedef struct rt_stats {
    double kernel_ms;            /* last rt_render: trace kernel time (HIP events) */
    double reduce_ms;            /* last rt_render: chunk-reduction kernel time */
    uint64_t samples;
    uint64_t casts;              /* count_work only */
    uint64_t node_visits;        /* count_work only: BVH nodes fetched */
    uint64_t prim_tests;         /* count_work only */
    uint64_t n_items;            /* work items (pixel, chunk) */
    int32_t n_chunks, spp_chunk;
    int64_t scene_bytes;         /* device bytes of the uploaded scene */
    int32_t node_bytes, prim_bytes, material_bytes;
    int32_t variant_features;    /* feature set of the kernel variant launched */
    int32_t slab32;              /* 1 if the conservative f32 slab test was used */
    int32_t lds_stack;           /* 1 if the traversal stack lived in LDS */
    int32_t lds_nodes;           /* TLAS nodes kept in LDS (0: read from L1/L2) */
    uint64_t cycles_camera;      /* count_work only: wave-cycles in camera-ray generation */
    uint64_t cycles_trace;       /* count_work only: wave-cycles in traversal + hit records */
    uint64_t cycles_shade;       /* count_work only: wave-cycles in materials / textures */
    uint64_t wave_steps;         /* count_work only: bounce-loop iterations executed per wave, summed;
                                    casts / (64 * wave_steps) = lane occupancy of the bounce loop */
    uint64_t wave_node_steps;    /* count_work only: node-visit iterations per wave, summed;
                                    node_visits / (64 * wave_node_steps) = its lane occupancy */
    uint64_t cycles_nodes;       /* count_work only: wave-cycles in BVH node-visit loops (part of trace) */
    uint64_t cycles_leaves;      /* count_work only: wave-cycles in leaf primitive tests (part of trace) */
    int32_t schedule;            /* RT_SCHED_* the last render ran with */
    int32_t n_batches;           /* trace launches it took (pool: per-sample buffer batches) */
    uint64_t wave_leaf_steps;    /* count_work only: leaf-loop iterations per wave, summed;
                                    prim_tests / (64 * wave_leaf_steps) = its lane occupancy */
    uint64_t camera_lanes;       /* count_work only: lanes starting a sample, summed over the */
    uint64_t camera_steps;       /*   wave iterations in which any lane did (camera_steps) */
    uint64_t shade_lanes;        /* count_work only: lanes shading a hit, summed over the */
    uint64_t shade_steps;        /*   wave iterations in which any lane did (shade_steps) */
    int32_t precision;           /* RT_PREC_* the last render ran with */
    int32_t waves_per_simd;      /* resident waves per SIMD of the last trace kernel (occupancy) */
    int64_t trace_buf_bytes;     /* the trace-output buffer the last render used (both halves when overlapped) */
    int32_t overlapped;          /* 1 if its buffer batches ran overlapped (two trace streams) */
    int32_t reserved0;           /* always 0 (ABI v4's wavefront-schedule iteration count; that schedule is gone) */
    int64_t ring_bytes;          /* POOL with the in-kernel reduction (ABI v3): its record ring, part of
                                    trace_buf_bytes; 0 when the per-sample buffer ran */
    /* RT_OPT_PRIMARY_CANDIDATES (additive to ABI v6): the per-pixel candidate table the last render's
     * new samples took their first hit from; all 0 when the render walked every primary ray */
    int64_t primary_table_bytes; /* 16 B per image pixel */
    double primary_build_ms;     /* its build inside this render (0: reused from the context's cache) */
    double primary_walk_share;   /* share of the image's pixels flagged "walk" (their primary rays walk) */
    /* RT_OPT_SKIP_SKY_TILES (additive to ABI v6) */
    int64_t sky_tiles;           /* 8x8 tiles the last render did not trace: every pixel of them sees only the
                                    background (0: the option off, or a render it does not apply to) */
    /* RT_OPT_DEFER_ROOTS (additive to ABI v6) */
    int64_t defer_roots;         /* 1: the last render's trace kernel was the primary-candidate kernel with deferred
                                    sphere roots; 0: any other kernel (the option off, or no primary-candidate table) */
} rt_stats;
int rt_last_stats(rt_ctx* ctx, rt_stats* out);

/* The candidate table of RT_OPT_PRIMARY_CANDIDATES built on the host (no device): for image pixel
 * (x, y), row 0 = bottom, records[8 * (y * width + x)] is the candidate count n (0xffff: the pixel
 * is flagged "walk") and the next n entries are leaf slots of the flattened scene (prim_refs[slot]
 * is the primitive). Every primitive a primary ray of the pixel can hit is in its list, for any
 * jitter, lens point and ray time of the camera. k_max: candidates before a pixel is flagged. */
typedef struct rt_primary_candidates_info {
    int64_t pixels, flagged;     /* pixels of the frame, and those flagged "walk" */
    int64_t candidates;          /* candidates summed over the pixels not flagged */
    int32_t max_candidates;      /* the longest list */
    int32_t slots;               /* candidates a record can hold (7) */
} rt_primary_candidates_info;
int rt_primary_candidates_host(const rt_scene_soa* scene, const rt_camera* cam, int width, int height, int k_max,
                               uint16_t* records, rt_primary_candidates_info* info);
/* The all-sky 8x8 tiles of that table (RT_OPT_SKIP_SKY_TILES; no device): flags[ty * ceil(width / 8) + tx]
 * is 1 when every pixel of raster tile (tx, ty) within the frame has an empty candidate list (n == 0),
 * else 0; ceil(width / 8) * ceil(height / 8) bytes. *count (optional) is how many are 1. */
int rt_primary_sky_tiles_host(const rt_scene_soa* scene, const rt_camera* cam, int width, int height, int k_max,
                              uint8_t* flags, int64_t* count);
/* Diagnostic: the raw count_work counters of the last render (n entries; returns how many
 * exist). 0-14 as in rt_stats; wave-cycles (s_memtime) per phase of the pool kernels: 3 ray
 * generation, 4 trace, 5 shading, 8 node loops, 9 leaf tests (both of the top-level walk),
 * 15 ray set-up, 16 walk prologue (pre-leaf test), 17 hit record, 18 media and 19 instances
 * (inside the leaf tests), 20 refill, 21 kernel total (summed over waves), 22 deferred instance
 * walks (after the top-level walk), 23 / 24 ray generation's seeding + jitter / rejection loop, 25
 * the longest wave lifetime, 26 waves. Bounce-loop lane slots that cast nothing (with casts they
 * add up to 64 x wave_steps): 27 idle, no unit left (the tail), 28 idle, every ring slot holding
 * an unfinished block, 29 the path ended in its scatter, 30 the depth cap, 31 a rejection loop
 * carried to the next iteration. */
int rt_last_counters(rt_ctx* ctx, uint64_t* out, int n);

/* ---- tile order: balancing tile shards (ABI v4; main.rs:497-551's partition, rebalanced) ------ */
/* Per 8x8 tile of the image (raster order, ceil(width/8) per tile row), the lane-cycles
 * (s_memtime) its samples took in the last render, if that render had count_work set and ran
 * a pool schedule (POOL, ITEMS; any shard mode). Copies min(n, tiles) entries; returns the
 * tile count, or 0 when the last render counted none. A cost estimate for
 * rt_ctx_set_tile_order: e.g. a few samples per pixel of the frame with count_work. */
int rt_last_tile_costs(rt_ctx* ctx, uint64_t* out, int64_t n);
/* The order in which tile shards (rt_render_params.tile_shard = 1) take the frame's tiles:
 * order[t] is the raster tile at position t, a permutation of the frame's n tiles (checked:
 * RT_ERR_INVALID otherwise). Shards then take positions row_begin + m*row_stride; a frame of
 * another tile count fails with RT_ERR_INVALID. Under a tile order the pool schedules also deal
 * their work blocks tile-major (all of a tile's sample groups before the next tile's) instead
 * of sample-group-major. The tiles sorted by cost, most expensive first, then give round-robin
 * shards of nearly equal cost, each finishing its expensive tiles first and ending on its
 * cheapest ones (a shard's launch otherwise ends on the last sample group of its most
 * expensive tiles). Only which pixels a shard renders, and when, changes, not their bits.
 * n = 0: raster order again (the default). Waits for the device.
 *
 * Whole frames need no such call (RT_OPT_AUTO_DEAL_ORDER, default on): a render that is not a
 * tile or row shard, not count_work, not an rt_render_adaptive pass, on a pool schedule (POOL with
 * its buffer or its ring, ITEMS; every buffer batch; f64 and f32) is dealt tile-major in a cost
 * order the context measures for itself. The first such render of a (scene upload, camera, width,
 * height) runs tile-major in raster order while its trace kernel adds, per work block, the wave's
 * cycles until its next block fetch to the block's tile; the second reads those costs back once
 * (8 bytes per tile, one stream synchronization inside that call), sorts them as
 * rt_cost_tile_order does and uploads the order; every later one, at any spp, seed, depth or
 * sample range (rt_accum_add, rt_render_progressive), reuses it with no host work. Only the order
 * blocks are handed out in changes: records, the reduction and the frame stay raster, so no bit
 * changes. A new upload or another key drops the order. The spheres kernel variants carry it
 * (scenes of spheres and moving spheres: the random scenes); scenes on the other variants keep
 * raster order. This context order (rt_ctx_set_tile_order) and the tile shards
 * it serves are not affected. */
int rt_ctx_set_tile_order(rt_ctx* ctx, const uint32_t* order, int64_t n);
/* The order the last render was dealt in under RT_OPT_AUTO_DEAL_ORDER: copies min(n, tiles)
 * entries (position -> raster tile) and returns the tile count, or 0 when it was dealt in raster
 * order (a key's first render, an ineligible render, option 0 or 2). */
int rt_last_deal_order(rt_ctx* ctx, uint32_t* out, int64_t n);

/* ---- multi-GPU render: tile shards, one RCCL gather, on-device reassembly (ABI v5) ------------
 * The reference splits one frame over 10 threads (main.rs:497-551: every thread all pixels,
 * spp/10 samples) and merges their buffers under a mutex (main.rs:542-547). Here a frame is split
 * over GPUs by 8x8 tiles: rank r of `world` renders the tiles at positions r, r + world, ... of the
 * frame's tile order (rt_render_params.tile_shard), RCCL gathers every rank's slab to rank 0 over
 * xGMI in one collective, and a reorder kernel on rank 0 writes the frame. Every draw is keyed by
 * (pixel, sample), so in RT_PREC_F64 the frame is bit-identical to rt_render's at any world size
 * and tile order. In RT_PREC_F32 the bits depend on the trace kernel that ran (rt_ctx_set_precision):
 * the frame is rt_render's bit for bit whenever the shards and the whole frame take the same one
 * (a forced schedule, and the same choice of POOL's ring or buffer), at any world size and tile
 * order; under RT_SCHED_AUTO a shard that fits the buffer bound where the whole frame does not may
 * take another kernel, and then agrees with it statistically only.
 *
 * A communicator binds one context (one device) to one rank. Two ways to make them:
 *   one process per GPU:     rank 0 calls rt_comm_unique_id and sends the 128 bytes to the other
 *                            ranks (any channel: MPI, a socket, torch.distributed); every rank then
 *                            calls rt_comm_init_rank with its own context (ncclCommInitRank);
 *   one process, N GPUs:     rt_comm_init_all over N contexts on N distinct devices
 *                            (ncclCommInitAll), then the *_all calls drive every rank from one
 *                            host thread (RCCL group calls).
 * RCCL (librccl.so.1) is loaded when the first communicator is made; the rest of the library does
 * not need it. Collective calls (rt_comm_tile_order, rt_render_gather) must be made by every rank
 * of the communicator with the same camera and frame parameters. */
typedef struct rt_comm rt_comm;
enum { RT_COMM_ID_BYTES = 128 };   /* ncclUniqueId */
int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
int rt_comm_init_rank(rt_ctx* ctx, int rank, int world, const uint8_t id[RT_COMM_ID_BYTES], rt_comm** out);
int rt_comm_init_all(rt_ctx* const* ctxs, int n, rt_comm** comms_out);
/* Destroys the RCCL communicator (after the rank's enqueued work is done); the context stays. */
void rt_comm_destroy(rt_comm* comm);
int rt_comm_rank(const rt_comm* comm, int* rank, int* world);

/* Collective: the cost-ordered tile deal (rt_ctx_set_tile_order) on every rank. Each rank renders
 * its raster-order tile shard of the frame p describes (its shard fields are ignored) at cost_spp
 * samples per pixel with count_work — f64 and a pool schedule, whatever the context is set to —
 * one RCCL all-reduce sums the per-tile lane-cycles (each tile counted by one rank), and every
 * rank sets the same order, rt_cost_tile_order's, on its context. A rank whose pass fails (and,
 * with RT_ERR_PEER, every other rank) falls back to raster order. The cost pass is 1/world of a
 * cost_spp frame per rank. */
int rt_comm_tile_order(rt_comm* comm, const rt_camera* cam, const rt_render_params* p, int cost_spp);
int rt_comm_tile_order_all(rt_comm* const* comms, int n, const rt_camera* cam, const rt_render_params* p,
                           int cost_spp);

/* Collective: one frame over the communicator's ranks. p describes the whole frame (its shard
 * fields row_begin / row_stride / row_block / tile_shard are ignored: rank r renders the tile
 * shard r of `world` in the context's tile order). Rank 0 receives the frame (height x width x 3
 * of p->out_format, row 0 = bottom), as rt_render's: on the device if p->out_on_device (the work
 * is then only enqueued on p->stream or the context's stream), else in host memory (synchronous).
 * Other ranks ignore `frame` (may be NULL) and, without out_on_device, return once their slab
 * has been sent. */
int rt_render_gather(rt_comm* comm, const rt_camera* cam, const rt_render_params* p, void* frame);
/* The same for the n ranks of one process (rt_comm_init_all; comms[i] is rank i): every rank's
 * render is enqueued on its context's stream, then the n gathers as one RCCL group. p->stream must
 * be NULL; with out_on_device, frame is a device pointer on comms[0]'s device. */
int rt_render_gather_all(rt_comm* const* comms, int n, const rt_camera* cam, const rt_render_params* p,
                         void* frame);

typedef struct rt_comm_stats {
    double render_ms;     /* last rt_render_gather: this rank's shard render (HIP events on its stream) */
    double gather_ms;     /* its RCCL gather: from the end of its render to the gather's end (includes the
                             wait for slower ranks) */
    double assemble_ms;   /* rank 0: the reorder kernel */
    double kernel_ms;     /* the trace kernel's part of render_ms (rt_stats.kernel_ms) */
    int64_t slab_bytes;   /* bytes each rank sent (its slab, padded to the largest shard) */
    int32_t tiles;        /* this rank's tiles */
    int32_t tile_order;   /* 1: a cost order was set by the last rt_comm_tile_order; 0: raster */
    double cost_pass_ms;  /* last rt_comm_tile_order on this rank: wall time of the count pass + all-reduce */
    int32_t peer_failed;  /* rank 0: ranks whose shard render failed in the last gather (their status words,
                             sent with the slabs; a host-bound rt_render_gather returns RT_ERR_PEER then) */
} rt_comm_stats;
int rt_comm_last_stats(rt_comm* comm, rt_comm_stats* out);

/* The reorder kernel alone, for callers with their own transport: `world` tile slabs at
 * `slabs` (device memory of ctx's device, rank r's at r * slab_elems elements; slab_elems >=
 * 8 * 8 * rt_tiles_in_shard(width, height, 0, world) * 3) -> frame (device, height x width x 3) of
 * p->out_format for the frame p describes, in ctx's tile order. Enqueued on p->stream (or the
 * context's stream). */
int rt_tiles_assemble(rt_ctx* ctx, const void* slabs, int64_t slab_elems, int world, const rt_render_params* p,
                      void* frame);
/* The same on the host (no device): elem_bytes 4 (f32) or 8 (f64), order NULL (raster) or the
 * n-tile permutation rt_ctx_set_tile_order takes. */
int rt_tiles_assemble_host(const void* slabs, int64_t slab_elems, int world, int width, int height, int elem_bytes,
                           const uint32_t* order, void* frame);
/* The cost order from per-tile costs (rt_last_tile_costs): raster tiles sorted by cost, most
 * expensive first, ties in raster order. Host only. */
int rt_cost_tile_order(const uint64_t* costs, int64_t n, uint32_t* order);

/* ---- progressive / resumable accumulation ------------------------------------ */
/* A device f64 running sum per pixel of one row shard. Batches render consecutive sample
 * ranges [done, done + n) and add their per-pixel sums; rt_accum_resolve divides. When
 * every batch boundary is a multiple of the chunk size (rt_render_params.spp_chunk at
 * create time; 0 = rt_render's auto choice for p->spp), the result is bit-identical to
 * one rt_render of the same total spp: the sums are added in the same order.
 * The reference's version of this is each thread's local_pixel_colors merged into the
 * mutex-guarded buffer (main.rs:508-547) plus the progress channel (main.rs:504-582). */
typedef struct rt_accum rt_accum;
/* p: width, height, row_begin, row_stride, spp (for the auto chunk) and spp_chunk. */
int rt_accum_create(rt_ctx* ctx, const rt_render_params* p, rt_accum** out);
void rt_accum_destroy(rt_accum* acc);
/* Renders samples [done, done + sample_count) of the shard with p's camera-independent
 * settings (max_depth, background, render_seed, count_work, stream; its geometry fields
 * must match the accumulator's) and adds them. Enqueued on the stream; rt_last_stats
 * describes the batch. */
int rt_accum_add(rt_ctx* ctx, rt_accum* acc, const rt_camera* cam, const rt_render_params* p, int sample_count);
/* Checkpoint: samples done, and (if sums is not NULL) the rows_local x width x 3 f64 sums. */
int rt_accum_get(rt_accum* acc, double* sums, int64_t* samples_done);
/* Restore a checkpoint taken with rt_accum_get (same geometry and chunk size). */
int rt_accum_set(rt_accum* acc, const double* sums, int64_t samples_done);
/* out = sums * (1/divisor) (divisor 0: the samples done), as rt_render writes it. The
 * reference divides by its nominal spp even when spp/thread_count truncated the samples
 * actually taken (main.rs:516, 596): pass that spp as divisor to reproduce it. */
int rt_accum_resolve(rt_ctx* ctx, rt_accum* acc, double divisor, int out_format, int out_on_device, void* out);

/* Progress callback: return 0 to continue, nonzero to stop after this batch. */
typedef int (*rt_progress_fn)(void* user, int64_t samples_done, int64_t samples_total);
/* rt_render in batches of batch_spp samples (rounded up to the chunk size), calling
 * progress after each batch; out as rt_render (sums / samples done if stopped early). */
int rt_render_progressive(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, int batch_spp,
                          rt_progress_fn progress, void* user, void* out);

/* ---- tile-adaptive sampling (additive to ABI v6: new symbols only, RT_ABI_VERSION stays 6) ----
 * Every other render path spends p->spp samples on every pixel. rt_render_adaptive samples the
 * frame in passes and, after each pass, stops the 8x8 tiles whose estimate has converged; it also
 * hands back the per-tile sample counts and a per-pixel noise estimate. Every draw is keyed by
 * (pixel, sample), so a tile that stopped at n samples holds exactly rt_render's pixels at spp = n
 * (same spp_chunk), bit for bit.
 *
 * The criterion. Per pixel, after its tile has n >= 2 samples:
 *   S      the RGB sum of its samples
 *   Y(c)   = 0.2126 r + 0.7152 g + 0.0722 b, in f64, evaluated left to right, no contraction
 *   Q      = sum over samples j of Y(sample_j)^2
 *   Ys     = Y(S),  m = Ys / n
 *   var    = max(0, (Q - Ys Ys / n) / (n - 1))
 *   se     = sqrt(var / n)                 the standard error of the luminance mean
 *   e_px   = se / sqrt(max(m, 1e-4))       the error after the output's sqrt gamma, up to the factor 1/2
 * Per tile: E_t = the mean of e_px over the tile's pixels inside the image (an edge tile counts
 * only those).
 * Stop rule, after every pass: a tile stops when E_t <= threshold or its count has reached p->spp
 * (the maximum); a stopped tile is never re-activated. threshold <= 0 never stops early; +inf
 * stops every tile at min_spp.
 * Sample counts: every tile gets min_spp samples first, active tiles then step_spp more per pass,
 * both rounded up to a multiple of the chunk (p->spp_chunk, or rt_render's automatic chunk for
 * p->spp, as rt_render_progressive); the last pass is cut at p->spp. All active tiles therefore
 * share one sample count, and a pass is one sample range [done, done + step).
 * Sum order: the RGB sums follow rt_render's (chunk sums from 0.0 in sample order, added in chunk
 * order); Q uses the same association.
 *
 * Each pass renders the active tiles as one tile shard under a tile order private to the call
 * ([every other tile | the active tiles]; the context's own order, rt_ctx_set_tile_order, is not
 * touched) on the POOL schedule's per-sample buffer, whatever the context is set to; buffer batches
 * (RT_OPT_TRACE_BUF_BYTES) carry the sums across. A moments kernel reduces the records into
 * frame-layout S and Q and the per-tile error, and a regroup kernel re-deals the tiles: the one an
 * rt_adaptive_state (below) chooses its groups with, the call being a fresh state advanced once to
 * (threshold, p->spp) and resolved.
 * p: the shard fields (row_begin, row_stride other than 0 / 1, row_block > 1, tile_shard) must be
 * unset (RT_ERR_INVALID); count_work is ignored; p->spp >= 2. RT_PREC_F32 contexts:
 * RT_ERR_UNSUPPORTED. One GPU. */
typedef struct rt_adaptive_params {
    int32_t min_spp;     /* >= 2: samples every tile gets before the first test (rounded up to the chunk) */
    int32_t step_spp;    /* >= 1: samples per later pass (rounded up to the chunk) */
    double threshold;    /* on E_t; <= 0: never stop early */
} rt_adaptive_params;

/* Host pointers, or device pointers if p->out_on_device. Tiles in raster order: ceil(width/8) per
 * tile row, t = ty * ceil(width/8) + tx, rows from the bottom as the frame's. */
typedef struct rt_adaptive_out {
    void* mean;            /* required: height x width x 3 of p->out_format, S * (1 / the tile's count) */
    uint32_t* tile_spp;    /* optional: samples per pixel each tile got */
    double* tile_error;    /* optional: E_t at the tile's last pass */
    double* stderr_map;    /* optional: height x width, se per pixel */
} rt_adaptive_out;

/* Synchronous, whether the outputs are host or device memory. */
int rt_render_adaptive(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, const rt_adaptive_params* ap,
                       const rt_adaptive_out* out);

typedef struct rt_adaptive_stats {
    int32_t passes;             /* passes of the last rt_render_adaptive */
    int32_t min_spp, step_spp;  /* as rounded to the chunk (min_spp at most p->spp) */
    int32_t spp_chunk;
    int32_t tiles;              /* tiles of the frame */
    int32_t max_pass_batches;   /* the most buffer batches one pass took */
    uint64_t samples_traced;    /* 64 x the sum of tile_spp over all tiles: an edge tile's pixels past the
                                   image are traced with it, as in every tile shard */
    uint64_t samples_uniform;   /* width x height x p->spp: what rt_render traces for the frame */
    double trace_ms;            /* HIP events, summed over passes: the trace kernels, */
    double moments_ms;          /*   the moments reductions, */
    double classify_ms;         /*   the regroup launches between and after the passes (with their readbacks) */
} rt_adaptive_stats;
int rt_adaptive_last_stats(rt_ctx* ctx, rt_adaptive_stats* out);

/* The adaptive frame plus its two half frames (additive to ABI v6: new symbols only), the input of
 * rt_denoise_cross. Everything rt_render_adaptive does, bit for bit: the same passes and stop
 * decisions, the same mean, tile_spp, tile_error and stderr_map, the same rt_adaptive_last_stats and
 * rt_last_stats conventions, the same errors (RT_PREC_F32 contexts: RT_ERR_UNSUPPORTED; one GPU,
 * whole frames); and halves NULL, either member NULL, or mean_a, mean_b and out->mean not three
 * different buffers: RT_ERR_INVALID.
 * The split. Half A holds the samples with an even global sample index s (the s of the (pixel, s)
 * key every draw has), half B the odd ones. A tile that stopped at n samples has n_a = (n + 1) / 2
 * and n_b = n / 2 of them.
 * The sums. S_a is summed as S is, restricted to its parity: per chunk, a half-sum starts from 0.0
 * and adds the chunk's samples of that parity in sample order; the chunk half-sums are added in
 * chunk order to 0.0. S_b likewise. mean_a = S_a * (1 / n_a), mean_b = S_b * (1 / n_b), in
 * p->out_format, height x width x 3, row 0 = bottom; device pointers iff p->out_on_device.
 * The bits do not depend on buffer batches (RT_OPT_TRACE_BUF_BYTES): the open chunk of each half is
 * carried across batches as S's is. At spp = min_spp = 2 mean_a is rt_render's frame at spp = 1.
 * The moments kernel's second instantiation carries the six half accumulators beside S and Q;
 * rt_render_adaptive keeps launching the first. */
typedef struct rt_adaptive_halves {
    void* mean_a;   /* required: the mean of the even samples */
    void* mean_b;   /* required: the mean of the odd samples */
} rt_adaptive_halves;
int rt_render_adaptive_halves(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p,
                              const rt_adaptive_params* ap, const rt_adaptive_out* out, const rt_adaptive_halves* halves);

/* The criterion above on the host, no device needed: sums (height x width x 3) and q (height x
 * width) are a frame's S and Q, tile_spp its per-tile sample counts (every one >= 2, else
 * RT_ERR_INVALID); writes E_t per raster tile to tile_error_out and se per pixel to stderr_out
 * (either may be NULL). For callers with accumulators of their own, and for tests. */
int rt_adaptive_tile_errors_host(const double* sums, const double* q, const uint32_t* tile_spp, int width,
                                 int height, double* tile_error_out, double* stderr_out);

/* ---- a resumable, refinable adaptive frame (additive to ABI v6: new symbols only) ----------------
 * rt_render_adaptive allocates its accumulators, runs to its threshold, resolves and frees them.
 * An rt_adaptive_state owns them between calls instead: S, Q, the half sums (with_halves),
 * tile_spp, tile_error and a tile order. It is advanced by rt_render_adaptive's trace passes and
 * moments kernel, so it can be tightened to a lower threshold, previewed between launches,
 * checkpointed, and steered by an error map of the caller's (a filter's error estimate reduced to
 * tiles, say). A tile's history depends on no other tile: every draw is keyed by (pixel, sample), a
 * tile only sits at counts of the schedule below, and it stops at the first of them where E_t <=
 * threshold.
 *
 * Create binds the camera, the context's current scene upload and p's width, height, max_depth,
 * background, render_seed and chunk (p->spp_chunk, or rt_render's automatic chunk for p->spp when
 * that is 0); the shard fields must be unset as for rt_render_adaptive; p->spp >= 1 only chooses
 * the automatic chunk. min_r and step_r are ap->min_spp (>= 2) and ap->step_spp (>= 1) rounded up
 * to the chunk; ap->threshold is ignored. The accumulators are zero and every tile has count 0.
 * RT_PREC_F32 contexts: RT_ERR_UNSUPPORTED, at create and at advance. A scene upload on the
 * context after create makes every later advance fail with RT_ERR_INVALID; the state can still be
 * resolved, read and destroyed. Destroy the state before its context (as an rt_accum).
 *
 * Schedule:  next(n) = min(spp_cap, n == 0 ? min_r : n + step_r).
 * Stops:     stops(E, threshold) = threshold > 0 and E <= threshold (rt_render_adaptive's
 *            predicate: a threshold <= 0 stops no tile, nor does a NaN E).
 * Active:    tile t with count n_t is active if n_t < spp_cap and (n_t == 0 or not
 *            stops(E_t, threshold)).
 * Advance:   until no tile is active, or max_launches groups have run:
 *              n* = the lowest count among the active tiles;
 *              the group = every active tile with count n*, in ascending raster index;
 *              samples [n*, next(n*)) of the group are traced as one tile shard under the state's
 *              own tile order [every other tile | the group], on the POOL schedule's per-sample
 *              buffer, exactly as a pass of rt_render_adaptive (buffer batches carry the sums
 *              across), and reduced by its moments kernel, which writes the group's tile_spp =
 *              next(n*) and E_t;
 *              one small record is read back (one synchronization per group).
 *            Every launch closes its last chunk: nothing is open between calls. *active_left =
 *            the active tiles after the call under this call's threshold and cap (may be NULL).
 *            The call is synchronous. On a fresh state run to completion the groups are exactly
 *            rt_render_adaptive's passes with the tiles in the same order (a stable partition of
 *            raster order stays ascending).
 * Ragged caps: a launch that ends at an spp_cap that is no multiple of the chunk closes a partial
 *            chunk. From then on an advance with a larger spp_cap is RT_ERR_INVALID before
 *            anything is launched (continuing would split that chunk's sum); the state remembers
 *            the cap on the host (and in its checkpoint). A cap below some tiles' counts is fine:
 *            those tiles are not active.
 * A caller's error map (tile_error_in not NULL, one f64 per raster tile; a device pointer if
 *            error_on_device): one round. The selected set is fixed at entry: the tiles with
 *            n_t < spp_cap and not stops(tile_error_in[t], threshold). Every selected tile gets
 *            exactly one step, to next(n_t); groups are formed by count, lowest first. A stepped
 *            tile's E_t is refreshed by the moments kernel, the others keep theirs.
 *            max_launches must be 0 and no tile may be at count 0 (RT_ERR_INVALID).
 *            *active_left = 0: the round always completes.
 * Resolve:   rt_render_adaptive's resolve on the state's sums: mean (out_format), tile_spp,
 *            tile_error, stderr_map and (halves) the two half means, to host pointers or (on_device)
 *            device pointers; synchronous, on the context's stream. RT_ERR_INVALID while a tile is
 *            at count 0, and for halves on a state created without them. It may be called between
 *            any two advances: a preview holds each tile at its own count.
 *
 * Consequences ("equals": every output bit for bit — the mean in both formats, tile_spp,
 * tile_error, stderr_map, mean_a and mean_b):
 *  1. A fresh state advanced to completion with (thr, cap) and resolved equals
 *     rt_render_adaptive(_halves) with spp = cap and the same chunk, min, step and threshold.
 *  2. advance(thr1), ..., advance(thrk) with decreasing thresholds equals one advance(thrk): the
 *     first scheduled count with E_t <= thrk cannot come before the first with E_t <= thr1.
 *  3. Any split of an advance by max_launches equals the unsplit advance.
 *  4. Raising the cap from c1 to c2 equals one run at cap c2, when c1 is on the schedule
 *     min_r + j step_r and a multiple of the chunk.
 *  5. get, set into a second state of the same create parameters, then continuing, equals
 *     continuing the first.
 *  6. After any sequence of calls a tile at count n holds rt_render's pixels at spp = n, same chunk.
 *
 * A regroup kernel (one 1024-thread workgroup, no atomics) chooses each group on the device; its
 * rule is stated once more on the host, rt_adaptive_next_group_host. rt_last_stats follows
 * rt_render_adaptive's convention for an advance; rt_adaptive_last_stats is not touched. The
 * context's tile order, schedule, options and deal-order cache are not touched. One GPU. */
typedef struct rt_adaptive_state rt_adaptive_state;
int rt_adaptive_state_create(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p,
                             const rt_adaptive_params* ap, int with_halves, rt_adaptive_state** out);
void rt_adaptive_state_destroy(rt_adaptive_state* st);

typedef struct rt_adaptive_advance_params {
    double threshold;             /* as rt_adaptive_params.threshold (NaN: RT_ERR_INVALID) */
    int32_t spp_cap;              /* >= 2: the most samples a tile may hold after this call */
    int32_t max_launches;         /* 0: until no tile is active; k > 0: at most k groups */
    int32_t error_on_device;      /* tile_error_in is a device pointer */
    int32_t reserved0;
    const double* tile_error_in;  /* optional, one value per raster tile: a caller's error map */
    void* stream;                 /* NULL: the context's stream */
} rt_adaptive_advance_params;
int rt_adaptive_state_advance(rt_adaptive_state* st, const rt_adaptive_advance_params* ap, int32_t* active_left);

/* out->mean is required, the others optional (rt_adaptive_out); halves NULL, or both members set. */
int rt_adaptive_state_resolve(rt_adaptive_state* st, int out_format, int on_device, const rt_adaptive_out* out,
                              const rt_adaptive_halves* halves);

/* A checkpoint on the host. The header names what a restore must match and carries the host side
 * of the state; the arrays are the frame-layout accumulators (nothing is open between calls). */
typedef struct rt_adaptive_state_header {
    int32_t width, height;
    int32_t spp_chunk, min_spp, step_spp;   /* as rounded: min_r, step_r */
    int32_t with_halves;
    int32_t ragged_cap;                     /* 0, or the cap at which a partial chunk was closed */
    int32_t reserved0;
    uint64_t groups_total, samples_total;   /* as rt_adaptive_state_stats */
} rt_adaptive_state_header;
typedef struct rt_adaptive_state_data {
    double* sums;         /* height x width x 3: S */
    double* q;            /* height x width: Q */
    uint32_t* tile_spp;   /* per raster tile */
    double* tile_error;   /* per raster tile */
    double* sum_a;        /* height x width x 3 each; with_halves only, else ignored */
    double* sum_b;
} rt_adaptive_state_data;
/* header (required) and, if data is not NULL, every array of it (all required; sum_a / sum_b only
 * with halves). Host pointers. */
int rt_adaptive_state_get(rt_adaptive_state* st, rt_adaptive_state_header* header, const rt_adaptive_state_data* data);
/* Restores a checkpoint: width, height, spp_chunk, min_spp, step_spp and with_halves must be the
 * state's own; every count is 0 or >= 2, and a multiple of the chunk or the header's ragged_cap
 * (RT_ERR_INVALID otherwise, the state unchanged). */
int rt_adaptive_state_set(rt_adaptive_state* st, const rt_adaptive_state_header* header,
                          const rt_adaptive_state_data* data);

typedef struct rt_adaptive_state_stats {
    int32_t groups;             /* groups traced by the last advance */
    int32_t active_left;        /* active tiles after it, under its threshold and cap */
    int32_t min_count, max_count;   /* the lowest and the highest tile count now */
    int32_t spp_chunk, min_spp, step_spp;   /* as rounded */
    int32_t tiles;              /* tiles of the frame */
    uint64_t samples_traced;    /* by the last advance: 64 x tiles x samples, summed over its groups */
    uint64_t groups_total, samples_total;   /* since create (or as restored) */
    double trace_ms;            /* the last advance, HIP events summed over its groups: the trace kernels, */
    double moments_ms;          /*   the moments reductions, */
    double classify_ms;         /*   the regroup launches (with their readback) */
} rt_adaptive_state_stats;
int rt_adaptive_state_last_stats(rt_adaptive_state* st, rt_adaptive_state_stats* out);

/* The selection rule on the host, no device needed: the next group of a frame with the given
 * counts. Give tile_error (the threshold decides, as in an advance) or selected (one byte per tile,
 * nonzero = selected, as in a caller's-map round: threshold is ignored), not both. min_r and step_r
 * are multiples of the chunk already. group_out (may be NULL; room for n_tiles) receives the
 * group's raster indices in ascending order. No active tile: n_group = 0, n_star = n_next = 0. */
typedef struct rt_adaptive_group {
    int64_t n_group;    /* tiles of the group */
    int64_t n_active;   /* active tiles, the group's included */
    int32_t n_star;     /* the group's count */
    int32_t n_next;     /* next(n_star) */
} rt_adaptive_group;
int rt_adaptive_next_group_host(const uint32_t* tile_spp, const double* tile_error, const uint8_t* selected,
                                int64_t n_tiles, double threshold, int32_t spp_cap, int32_t min_r, int32_t step_r,
                                uint32_t* group_out, rt_adaptive_group* out);

/* ---- variance-guided NL-means denoiser (additive to ABI v6: new symbols only) ------------------
 * A post-filter for rt_render_adaptive's frame that needs only the colour and the per-pixel
 * standard error the adaptive call already returns: non-local means with variance-normalised
 * patch distances (Rousselle, Knaus, Zwicker 2012). No albedo, normal or depth buffer, no uploaded
 * scene, no scratch buffer: it reads mean and stderr_map and writes out.
 *
 * The filter. Inputs: M, height x width x 3 mean radiance (f32 or f64, row 0 = bottom); se, height
 * x width f64 (rt_adaptive_out.stderr_map); radius r in 1..10; patch f in 0..3; k > 0 and finite.
 * All arithmetic is f64 with no contraction; f32 input is widened first.
 *   Y(a)     = the luminance of M(a), by rt_render_adaptive's expression for Y
 *   V(a)     = se(a)^2
 * For a pixel a and an offset o in [-r, r]^2 the pair (a, o) is valid if a and a + o are both inside
 * the image.
 *   delta(a, o) = ((Y(a) - Y(a+o))^2 - (V(a) + min(V(a), V(a+o)))) / (1e-10 + k^2 (V(a) + V(a+o)))
 *   D(p, o)     = the sum of delta(p+s, o) over the s in [-f, f]^2 whose pair (p+s, o) is valid,
 *                 divided by the number of such s
 *   w(p, o)     = exp(-max(0, D)) if D is finite, otherwise 0; w(p, (0,0)) = 1 by definition
 *   out(p)      = sum_o w(p,o) M(p+o) / sum_o w(p,o) over the offsets with p + o inside the image,
 *                 taken in raster order (dy outer, dx inner); terms with w = 0 are skipped, not
 *                 multiplied
 * If Y(p) or V(p) is not finite, out(p) = M(p): with the finite-D rule a NaN or Inf pixel stays
 * where it is and does not spread. out has M's format; an f32 out is the f64 result rounded once.
 * The patch sums are direct sums of their (2f+1)^2 terms (no running sums or integral images:
 * where V = 0, delta reaches 1e10 and a running sum loses the small terms next to it). The distance
 * is not symmetric in (a, a+o). Nothing depends on the device's tiling: the result repeats bit for
 * bit, and the device and host filters differ only by their exp (an ulp of a weight). */
typedef struct rt_denoise_params {
    int32_t width, height;
    int32_t format;      /* RT_OUT_F32 / RT_OUT_F64, of mean and out */
    int32_t on_device;   /* 0: host pointers, synchronous; 1: device pointers, only enqueued */
    int32_t radius, patch;
    double k;
    void* stream;        /* hipStream_t (NULL = the context's stream) */
} rt_denoise_params;
/* RT_ERR_INVALID: a null pointer, out == mean, a bad format, width or height < 1, radius, patch or
 * k out of range. Needs no uploaded scene. With on_device set, rt_render_adaptive with
 * out_on_device followed by rt_denoise on the same stream runs with no host round trip. */
int rt_denoise(rt_ctx* ctx, const rt_denoise_params* p, const void* mean, const double* stderr_map, void* out);
/* The same filter on the host, no device needed (on_device and stream are ignored). */
int rt_denoise_host(const rt_denoise_params* p, const void* mean, const double* stderr_map, void* out);

typedef struct rt_denoise_stats {
    double kernel_ms;        /* last rt_denoise: the filter kernel (HIP events; waits for it if only enqueued) */
    int32_t radius, patch;
    int32_t lds_bytes;       /* LDS of one workgroup (one 16x16 tile) */
    int32_t reserved0;
} rt_denoise_stats;
int rt_denoise_last_stats(rt_ctx* ctx, rt_denoise_stats* out);

/* ---- first-hit feature buffers (additive to ABI v6: new symbols only) ---------------------------
 * The auxiliary buffers a denoiser takes beside the colour: per pixel the mean, over the pixel's
 * p->spp samples, of the first hit's albedo, normal and depth. One GPU, whole frames, f64.
 *
 * Which ray. For every pixel and every sample s in [0, p->spp) the primary ray is exactly the one
 * rt_render shoots for (pixel, s) under p->render_seed: the same path stream and the same camera
 * ray, pixel jitter, lens draw and time draw included. It is cast once, as rt_render's first
 * bounce is (t_min = 0.001, the medium's draw keyed by bounce 0, so fog is hit where rt_render's
 * path hits it). Nothing scatters, no scatter value is drawn and no second ray is cast.
 *
 * What a sample contributes.
 *   albedo  the first hit's material colour at the hit record (its u, v, p): Lambertian and
 *           Isotropic their texture value (the attenuation their scatter returns), DiffuseLight
 *           its emitted texture value, Metal its albedo, Dielectric (1, 1, 1); a miss
 *           p->background
 *   normal  the hit record's world-space normal as the material sees it: against the ray
 *           (set_face_normal), mapped back through translate / rotate_y as the reference maps it;
 *           a constant medium's hit keeps the record's normal ((1, 0, 0) top-level, rotated and turned
 *           against the ray under an instance: rt_trace_rays, below); a miss (0, 0, 0)
 *   depth   sqrt((ex ex + ey ey) + ez ez), e = the hit point - the ray's origin; a miss 0
 * Sums. Every channel is sum * (1 / p->spp), the sum associated as rt_render's: chunk sums from
 * 0.0 in sample order, added in chunk order to 0.0; the chunk is p->spp_chunk, or rt_render's
 * automatic chunk for p->spp. Every draw is keyed by (pixel, sample), so the bits depend on
 * neither the launch geometry nor the acceleration structure nor the kernel variant. A mean
 * normal is shorter than 1 where the samples' normals differ.
 *
 * p: spp >= 1; max_depth, count_work and out_format are ignored; the shard fields (row_begin,
 * row_stride other than 0 / 1, row_block > 1, tile_shard) must be unset (RT_ERR_INVALID). No
 * uploaded scene: RT_ERR_NO_SCENE. RT_PREC_F32 contexts: RT_ERR_UNSUPPORTED. Host pointers: the
 * call is synchronous. With p->out_on_device the outputs are device pointers and the call is only
 * enqueued on p->stream (or the context's stream), like rt_render.
 * The kernel is trace_features (one instantiation per kernel variant, picked by the scene's
 * features and RT_OPT_EXTRA_FEATURES as rt_render's); chunk partials beyond
 * RT_OPT_TRACE_BUF_BYTES are taken in batches on chunk boundaries, same bits. */
typedef struct rt_features_out {      /* all f64, row 0 = bottom; at least one non-NULL */
    double* albedo;   /* height x width x 3, or NULL */
    double* normal;   /* height x width x 3, or NULL */
    double* depth;    /* height x width,     or NULL */
} rt_features_out;
int rt_render_features(rt_ctx* ctx, const rt_camera* cam, const rt_render_params* p, const rt_features_out* out);

typedef struct rt_features_stats {
    double kernel_ms, reduce_ms;   /* last rt_render_features: its trace_features launches, its reductions
                                      (HIP events; waits for them if the call was only enqueued) */
    uint64_t samples;              /* width x height x spp */
    int32_t variant_features;      /* the kernel variant's feature set, as rt_stats.variant_features */
    int32_t spp_chunk;
} rt_features_stats;
int rt_features_last_stats(rt_ctx* ctx, rt_features_stats* out);

/* ---- feature-guided NL-means (additive to ABI v6: new symbols only) -----------------------------
 * rt_denoise with its weight multiplied by a feature term, so a texture or geometry edge the
 * colour distance cannot tell from noise stays sharp. The filter is rt_denoise's in every respect
 * (D, the raster order of the offsets, the finite-value rules, out(p) = M(p) where Y(p) or V(p)
 * is not finite) except for the weight. Guides: A (albedo) and N (normal), height x width x 3 f64,
 * Z (depth), height x width f64, as rt_render_features writes them; each may be NULL. For a pixel
 * p and q = p + o, per pixel pair (not summed over the patch):
 *   a_i = A_i(p) - A_i(q);  dA = (a_0 a_0 + a_1 a_1) + a_2 a_2        (dN the same over N)
 *   z   = Z(p) - Z(q);      dZ = z z / (1e-10 + (Z(p) Z(p) + Z(q) Z(q)))
 *   Phi(p, o) = dA ia + dN in + dZ iz, left to right; ia = 1 / (sigma_albedo sigma_albedo) etc.,
 *               computed once on the host in f64; the term of a NULL guide is skipped
 *   w(p, o)   = exp(-(max(0, D(p, o)) + Phi(p, o))) if D and Phi are finite, otherwise 0;
 *               w(p, (0,0)) = 1
 * All arithmetic is f64 with no contraction. A NaN or Inf feature value at q therefore removes
 * the pairs that touch q and nothing else. g == NULL, or all three guides NULL, is rt_denoise bit
 * for bit (rt_denoise is this entry without guides). The guides are device pointers iff
 * p->on_device. RT_ERR_INVALID as rt_denoise, and for a non-NULL guide whose sigma is not greater
 * than 0 and finite; the sigma of a NULL guide is ignored. Albedo demodulation (filtering
 * colour / albedo) is not part of it. rt_denoise_last_stats reports a guided call as a plain one. */
typedef struct rt_denoise_guides {
    const double* albedo;   /* height x width x 3 or NULL */
    const double* normal;   /* height x width x 3 or NULL */
    const double* depth;    /* height x width or NULL */
    double sigma_albedo, sigma_normal, sigma_depth;   /* > 0 and finite for every non-NULL guide */
} rt_denoise_guides;
int rt_denoise_guided(rt_ctx* ctx, const rt_denoise_params* p, const void* mean, const double* stderr_map,
                      const rt_denoise_guides* g, void* out);
/* The same filter on the host, no device needed (on_device and stream are ignored). */
int rt_denoise_guided_host(const rt_denoise_params* p, const void* mean, const double* stderr_map,
                           const rt_denoise_guides* g, void* out);

/* ---- variance-guided a-trous wavelet denoiser (additive to ABI v6: new symbols only) ------------
 * A second filter beside rt_denoise, for noise broader than NL-means' 21 x 21 window or a frame
 * budget without milliseconds for a filter: the edge-stopping a-trous wavelet of Dammertz et al.
 * 2010 with the variance-scaled luminance stop of SVGF's spatial filter (Schied et al. 2017). L
 * levels of 25 taps at steps 1, 2, 4, ... cover a (4 (2^L - 1) + 1)^2 footprint (125 x 125 at
 * L = 5) with 25 L taps per pixel. The variance is carried through every level and handed back.
 *
 * Inputs: M, height x width x 3 mean radiance (f32 or f64, row 0 = bottom); se, height x width f64
 * (rt_adaptive_out.stderr_map); optional guides g (rt_denoise_guides with rt_denoise_guided's
 * meaning; NULL or all three frames NULL: no feature term); levels L in 1..6; sigma_l > 0 and
 * finite; demodulate 0 or 1. All arithmetic is f64 with no contraction and no fast math; f32 input
 * is widened first. Y(c) is the luminance of a colour c by rt_render_adaptive's expression.
 * State, per pixel: a colour C (3 channels) and a variance V.
 *   C_0 = M,  V_0 = se^2
 * With demodulate = 1 (needs a non-NULL albedo guide A), per channel c:
 *   A'_c(p) = A_c(p) if it is finite and > 0.01, 0.01 if it is finite and <= 0.01, 1 if it is not finite
 *   C_0,c = M_c / A'_c,  V_0 = se^2 / (Y(A') Y(A'))
 * A first-hit mean albedo demodulates a multi-bounce mean colour only approximately: the light a
 * path gathers after its first hit is tinted by later surfaces, and the mean of products is not the
 * product of means; C_0 is a smoother signal than M on a textured surface, not an irradiance.
 * Level i = 0..L-1, step s = 2^i, everything read from state i:
 *   Vbar(p) = the 3 x 3 binomial mean of V_i around p at distance 1 (not stepped), weights
 *             (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4), over the neighbours inside the image whose V_i is
 *             finite, divided by the sum of the weights taken, in raster order (dy outer, dx inner)
 *   dl(p)   = sigma_l sqrt(max(0, Vbar(p))) + 1e-10
 *   for the 25 taps q = p + s (dx, dy), dx, dy in -2..2, in raster order, with
 *   h = (1/16, 1/4, 3/8, 1/4, 1/16) and h(dx, dy) = h[dy+2] h[dx+2]:
 *     the centre tap has w = h(0, 0); a tap outside the image has no term; otherwise
 *     e = |Y(C_i(p)) - Y(C_i(q))| / dl(p) + Phi(p, q), Phi exactly rt_denoise_guided's term read from
 *         the guide frames at p and q (skipped without guides)
 *     w = h(dx, dy) exp(-e) if e and V_i(q) are finite, else 0; terms with w = 0 are skipped, not
 *         multiplied
 *   C_{i+1}(p) = sum w C_i(q) / sum w
 *   V_{i+1}(p) = sum w^2 V_i(q) / (sum w  sum w)
 *   If Y(C_i(p)) or V_i(p) is not finite, the pixel keeps C_i(p) and V_i(p): a NaN pixel stays where
 *   it is and does not spread.
 * Output: out = C_L, multiplied by A' per channel when demodulated; where Y(M(p)) or se(p) is not
 * finite, out(p) is M(p) bit for bit. The optional stderr_out (height x width f64) is sqrt(V_L),
 * V_L first multiplied by Y(A') Y(A') when demodulated: the standard error left in out's luminance
 * if the taps' errors were independent (they are not after the first level, so it is a lower
 * estimate). out has M's format; an f32 out is the f64 result rounded once. Nothing depends on the
 * device's tiling: the result repeats bit for bit, and the device and host filters differ only by
 * their exp. */
typedef struct rt_atrous_params {
    int32_t width, height, format, on_device;  /* as rt_denoise_params */
    int32_t levels, demodulate;
    double sigma_l;
    void* stream;        /* hipStream_t (NULL = the context's stream) */
} rt_atrous_params;
/* RT_ERR_INVALID as rt_denoise_guided returns it, and for out == mean, stderr_out == stderr_map,
 * levels, sigma_l or demodulate out of range, demodulate without an albedo guide. Needs no uploaded
 * scene. The guides, stderr_map and stderr_out are device pointers iff p->on_device; with it set the
 * call is only enqueued, like rt_denoise. The states between the first and the last level live in
 * scratch the context owns (none at L = 1, one frame of 32-byte records at L = 2, two above),
 * allocated on first need and grown when a larger frame arrives: a call that grows it may wait for
 * the stream, any other call with on_device set does no host-side wait. */
int rt_denoise_atrous(rt_ctx* ctx, const rt_atrous_params* p, const void* mean, const double* stderr_map,
                      const rt_denoise_guides* g, void* out, double* stderr_out /* may be NULL */);
/* The same filter on the host, no device needed (on_device and stream are ignored). */
int rt_denoise_atrous_host(const rt_atrous_params* p, const void* mean, const double* stderr_map,
                           const rt_denoise_guides* g, void* out, double* stderr_out /* may be NULL */);

typedef struct rt_atrous_stats {
    double kernel_ms;       /* last rt_denoise_atrous: its kernels, summed over levels (HIP events; waits if only enqueued) */
    int32_t levels;
    int64_t scratch_bytes;  /* state scratch that call used: 0, 1 or 2 x (32 width height) */
} rt_atrous_stats;
int rt_atrous_last_stats(rt_ctx* ctx, rt_atrous_stats* out);

/* ---- cross-filtered NL-means over two half frames (additive to ABI v6: new symbols only) ---------
 * rt_denoise's weights are computed from the very pixels they then average, so the noise of a weight
 * and the noise of the pixel it multiplies are correlated, and no output says how much error is
 * left. The dual-buffer answer of Rousselle, Knaus, Zwicker 2012: the pixel's samples are split into
 * two independent halves, each half is filtered with the weights taken from the other, the two
 * results are averaged, and the error left is read off their difference.
 *
 * Inputs: M_A and M_B, height x width x 3 mean radiance of the two halves (f32 or f64, row 0 =
 * bottom; e.g. the means over a pixel's even and over its odd samples); se, height x width f64, the
 * standard error of the whole mean (rt_adaptive_out.stderr_map); optional guides g
 * (rt_denoise_guides with rt_denoise_guided's meaning; NULL or all three frames NULL: no feature
 * term); radius r in 1..10; patch f in 0..3; k > 0 and finite; variance_scale > 0 and finite. All
 * arithmetic is f64 with no contraction and no fast math; f32 input is widened first.
 *   Y_h(a) = the luminance of M_h(a), h in {A, B}, by rt_render_adaptive's expression for Y
 *   V(a)   = variance_scale (se(a) se(a)): the variance of one half's luminance. A half of n / 2
 *            samples has twice the whole mean's variance, so halves of equal size take 2.0
 * A pixel a is bad if Y_A(a), Y_B(a) or V(a) is not finite; both Y_A and Y_B of a bad pixel count as
 * NaN, so no pair that touches it has a weight.
 *   delta_h(a, o), D_h(p, o): exactly rt_denoise's delta and D, from Y_h and V: the same valid-pair
 *            rule, the same division by the number of valid s, direct patch sums in the same order
 *   Phi(p, o): exactly rt_denoise_guided's feature term, the same for both halves; skipped without
 *            guides
 *   w_h(p, o) = exp(-(max(0, D_h(p, o)) + Phi(p, o))) if both are finite, otherwise 0;
 *            w_h(p, (0,0)) = 1
 * Cross application, over the offsets with p + o inside the image in raster order (dy outer, dx
 * inner), terms with w = 0 skipped, not multiplied:
 *   F_A(p) = sum_o w_B(p, o) M_A(p + o) / sum_o w_B(p, o)
 *   F_B(p) = sum_o w_A(p, o) M_B(p + o) / sum_o w_A(p, o)
 * A bad pixel keeps F_A(p) = M_A(p) and F_B(p) = M_B(p).
 *   out(p) = 0.5 (F_A(p) + F_B(p)) per channel
 * out has the means' format; an f32 out is the f64 result rounded once. The optional stderr_out
 * (height x width f64):
 *   e(p)  = 0.5 (Y(F_A(p)) - Y(F_B(p))),  E2(p) = e(p) e(p), from the unrounded F
 *   stderr_out(p) = sqrt of the 3 x 3 binomial mean of E2 around p by rt_denoise_atrous's Vbar rule:
 *           weights (1/4, 1/2, 1/4) x (1/4, 1/2, 1/4), over the neighbours inside the image whose E2
 *           is finite, divided by the sum of the weights taken, in raster order (dy outer, dx inner).
 *           Where E2(p) itself is not finite, stderr_out(p) = sqrt(E2(p)).
 * What stderr_out is: the standard error of out's luminance as far as the two halves disagree.
 * (F_A - F_B) / 2 has the variance of (F_A + F_B) / 2 when the halves are independent, and one
 * squared draw of it per pixel is smoothed over 3 x 3. That is out's variance, not its bias: both
 * halves share the blur of the filter, and it cancels in their difference. Where the filter
 * over-blurs, stderr_out understates the error.
 * With M_A = M_B = M and variance_scale = 1 the filter is rt_denoise (with guides rt_denoise_guided)
 * bit for bit on a frame whose se is finite everywhere (rt_denoise gives a pair whose far end has
 * se = Inf a delta of 0, the bad-pixel rule here gives it none), and stderr_out is 0. Swapping the halves changes no bit of out
 * or stderr_out. Nothing depends on the device's tiling: the result repeats bit for bit, and the
 * device and host filters differ only by their exp. */
typedef struct rt_cross_params {
    int32_t width, height, format, on_device;  /* as rt_denoise_params */
    int32_t radius, patch;
    double k;
    double variance_scale;   /* 2.0 for the two halves of an evenly split mean */
    void* stream;            /* hipStream_t (NULL = the context's stream) */
} rt_cross_params;
/* RT_ERR_INVALID as rt_denoise_guided returns it, and for a null mean_a or mean_b, out equal to one
 * of the inputs, stderr_out equal to stderr_map or to another frame of the call, variance_scale not
 * greater than 0 and finite. mean_a == mean_b is allowed. Needs no uploaded scene. Every pointer is a
 * device pointer iff p->on_device; with it set the call is only enqueued, like rt_denoise. With
 * stderr_out the kernel's e(p) goes through a height x width f64 scratch the context owns, allocated
 * on first need and grown when a larger frame arrives (a call that grows it may wait for the
 * stream), and a second small kernel takes the 3 x 3 rule; without it there is one launch and no
 * scratch. */
int rt_denoise_cross(rt_ctx* ctx, const rt_cross_params* p, const void* mean_a, const void* mean_b,
                     const double* stderr_map, const rt_denoise_guides* g /* may be NULL */, void* out,
                     double* stderr_out /* may be NULL */);
/* The same filter on the host, no device needed (on_device and stream are ignored). */
int rt_denoise_cross_host(const rt_cross_params* p, const void* mean_a, const void* mean_b, const double* stderr_map,
                          const rt_denoise_guides* g /* may be NULL */, void* out, double* stderr_out /* may be NULL */);

typedef struct rt_cross_stats {
    double kernel_ms;        /* last rt_denoise_cross: its one or two kernels (HIP events; waits if only enqueued) */
    int32_t radius, patch;
    int32_t lds_bytes;       /* LDS of one workgroup of the filter kernel: (3 SW^2 + 4 PW PS) 8 bytes, SW = 16 +
                                2 (radius + patch), PW = 16 + 2 patch, PS = 16 if patch == 0, else 48 */
    int32_t reserved0;
    int64_t scratch_bytes;   /* e scratch that call used: 0 without stderr_out, else 8 width height */
} rt_cross_stats;
int rt_cross_last_stats(rt_ctx* ctx, rt_cross_stats* out);

/* ---- multi-scale NL-means (additive to ABI v6: new symbols only) --------------------------------
 * The NL-means filters see at most a 21 x 21 window, so noise broader than the window survives as
 * low-frequency blotches. The pyramid answer (as in ray-histogram fusion, Delbracio et al. 2014):
 * the frame is reduced by 2 x 2 block means L - 1 times, rt_denoise_guided filters every level with
 * the same (radius, patch, k), and from the coarsest level down each level's result is corrected by
 * what the filtered coarser level knows better: its low frequencies. A window of radius r over L
 * levels covers a footprint of radius r 2^(L-1); the pixels of all levels sum to less than 4/3 of
 * the frame's.
 *
 * Inputs: M, se, the optional guides g, radius, patch and k exactly as rt_denoise_guided takes them;
 * levels L in 1..5. All arithmetic is f64 with no contraction and no fast math; f32 input is widened
 * first. "In raster order" means dy outer, dx inner, starting from 0.0.
 * Level frames. Level 0 is w_0 x h_0 = width x height; level l + 1 is w_{l+1} = (w_l + 1) / 2 by
 *   h_{l+1} = (h_l + 1) / 2 (integer division). A level may be 1 x 1.
 * Blocks. The block of a coarse pixel c = (cx, cy) is the set of level-l pixels (2 cx + i, 2 cy + j),
 *   i, j in {0, 1}, that lie inside the level-l frame; n is their number (1, 2 or 4) as a double.
 * Down. C_0 = M, s_0 = se. Per channel, C_{l+1}(c) = the raster-order sum of C_l over the block,
 *   divided by n. s_{l+1}(c) = sqrt(T) / n, T the raster-order sum of s_l(a) s_l(a) over the block:
 *   the standard error of a mean of independent pixels. Each guide frame given (A, N, Z) is reduced
 *   exactly as C is; the sigmas are every level's. Non-finite values get no special rule here: they
 *   go through the sums.
 * Per level. D_l = rt_denoise_guided's filter, exactly as its contract states it, on (C_l, s_l, the
 *   level's guides, radius, patch, k) at the level's size, kept in f64.
 * Up, for l = L - 2 down to 0, with R_{L-1} = D_{L-1}:
 *   B_l(c) = the block mean of D_l, by the Down rule
 *   K_l(c) = R_{l+1}(c) - B_l(c), per channel
 *   for a level-l pixel p = (x, y): cx = x / 2; ox = cx - 1 if x is even, else cx + 1, clamped to
 *   [0, w_{l+1} - 1]; cy and oy likewise from y and h_{l+1}. The taps, in this order: (cx, cy) with
 *   weight 9/16, (ox, cy) with 3/16, (cx, oy) with 3/16, (ox, oy) with 1/16; a clamped tap may repeat
 *   a pixel and is still taken. A tap is taken if all three channels of K_l there are finite.
 *   u(p) = (sum weight K_l) / (sum weight) over the taps taken, both sums in tap order from 0.0;
 *   u(p) = 0 if no tap is taken
 *   R_l(p) = D_l(p) + u(p)
 * Output: out = R_0 in M's format; an f32 out is the f64 value rounded once. Where Y(M(p)) or se(p)
 * is not finite, out(p) is M(p) bit for bit: a non-finite pixel stays where it is. A non-finite
 * colour makes K of the blocks that contain it non-finite at every level, which removes those
 * correction taps and nothing else; a pixel whose se alone is not finite is kept at every level
 * (s of its blocks is not finite either) and its blocks' K stays finite.
 * Consequences: L = 1 is rt_denoise_guided (without guides rt_denoise) bit for bit. Nothing depends
 * on the device's tiling: the result repeats bit for bit, and the device and host filters differ
 * only by their exp. */
typedef struct rt_pyramid_params {
    int32_t width, height, format, on_device;  /* as rt_denoise_params */
    int32_t radius, patch;                     /* as rt_denoise: 1..10, 0..3 */
    double k;                                  /* > 0 and finite */
    int32_t levels;                            /* L in 1..5 */
    int32_t reserved0;                         /* must be 0 */
    void* stream;        /* hipStream_t (NULL = the context's stream) */
} rt_pyramid_params;
/* RT_ERR_INVALID as rt_denoise_guided returns it, and for levels outside 1..5 or reserved0 != 0.
 * Needs no uploaded scene. Every pointer is a device pointer iff p->on_device; with it set the call
 * is only enqueued, like rt_denoise. At L = 1 the call is rt_denoise_guided's one launch on the
 * caller's buffers and uses no scratch. At L >= 2 the levels' f64 frames (C_l, s_l, the guides given
 * and D_l of every level above 0, D_0, the widened frame when M is f32, and one K frame of level
 * 1's size) live in scratch the context owns, allocated on first need and grown when a call needs
 * more: a call that grows it may wait for the stream, any other call with on_device set does no
 * host-side wait. The filters of the levels above 0 are too few workgroups to fill a device, so
 * they run on a stream of the context's own beside level 0's, ordered after Down and before Up by
 * events: all of the call's work is complete when what it enqueued on its stream is. */
int rt_denoise_pyramid(rt_ctx* ctx, const rt_pyramid_params* p, const void* mean, const double* stderr_map,
                       const rt_denoise_guides* g /* may be NULL */, void* out);
/* The same filter on the host, no device needed (on_device and stream are ignored). */
int rt_denoise_pyramid_host(const rt_pyramid_params* p, const void* mean, const double* stderr_map,
                            const rt_denoise_guides* g /* may be NULL */, void* out);

typedef struct rt_pyramid_stats {
    double kernel_ms;        /* last rt_denoise_pyramid: all its kernels (HIP events; waits if only enqueued) */
    int32_t levels, radius, patch;
    int32_t reserved0;
    int64_t scratch_bytes;   /* level scratch that call used: 0 exactly when levels == 1 */
} rt_pyramid_stats;
int rt_pyramid_last_stats(rt_ctx* ctx, rt_pyramid_stats* out);

/* ---- ray queries: closest hit and occlusion of caller rays (additive to ABI v6: new symbols only) --
 * The walk rt_render makes for its own rays, for rays the caller states: one cast per ray, nothing
 * scatters, no path value is drawn. One GPU, f64.
 *
 * Closest. RT_QUERY_CLOSEST is hit_hittables(world, ray, t_min, t_max) (hittable.rs:43-55) and the
 * HitRecord of the closest primitive. The two interval ends are handed to every primitive test
 * unchanged, so every interval edge case is whatever that test does with them (hittable.rs:254-273,
 * 308-320, 417-473). With t_min = 0.001, t_max = +inf, bounce = 0 and the key (pixel, sample) it is
 * the cast rt_render and rt_render_features make for that pixel's sample, bit for bit
 * (rt_camera_rays writes those rays). Closest hit does not depend on the order of the tests, and
 * the one draw of a cast, a constant medium's, is keyed by (seed, key_pixel, key_sample, bounce): the
 * bits of a ray's result depend on that ray and the scene alone — not on the launch, the order of
 * the rays in the array, the batches a call is taken in, the acceleration structure or the kernel
 * variant. Where two top-level primitives accept exactly the same t (coincident faces: the final
 * scene's ground boxes tile a grid and share their sides; a test rejects t > t_max only), the record
 * is that of the one later in rt_scene_soa.prims, which is the later entry of the world's list and
 * the one hit_hittables' loop keeps, under every acceleration structure. (rt_render's and
 * rt_render_features' casts keep the record of the later test instead, so under RT_ACCEL_SAH they
 * may shade the other of two such primitives; t and p are the same. Two primitives of one
 * instance's BVH with the same t: inner is either, as for a medium bounded by a BVH, below.)
 *   t       in units of d (d is not normalised, as the reference's); +inf: a miss
 *   p, n    the record's point and normal: n against the ray (set_face_normal), both mapped back
 *           through translate / rotate_y as the reference maps them, every level applying
 *           set_face_normal again (hittable.rs:232-244, 386-415: a hit from inside an instanced box
 *           is front-facing). A top-level medium's hit keeps the record's (1, 0, 0) and front_face;
 *           a medium under an instance gets that normal rotated and turned against the ray like
 *           any other: +-(cos a, 0, -sin a) under translate(rotate_y(., a)), the sign from d.
 *           A miss: zeros
 *   prim    index in rt_scene_soa.prims of the top-level primitive; -1 on a miss. Top-level as the
 *           tables have it: an entry of the world's list is one record, except an rt_world_bvh
 *           pushed as it is and an instance over a BVH that holds more than plain primitives, whose
 *           members are top-level records of their own (the instance's ops pushed down to each)
 *   inner   the geometric primitive behind t: prim itself, the child or BLAS primitive of an
 *           instance, the boundary of a medium (through the boundary's instance, if it has one; a
 *           boundary that is a BVH is a set, and inner is then one primitive of it — which one
 *           depends on the acceleration structure, the one field of a record that does); -1 on a miss
 *   mat     the material index the record carries (a medium: its phase function); -1 on a miss
 *   flags   RT_HIT_FRONT: the record's front_face; RT_HIT_MEDIUM: the record is a constant medium's
 *   albedo  (rt_query_out.albedo) the colour rt_render_features' albedo names for the record; a
 *           miss: zeros (not a background: a query has none). A caller's rays choose the point a
 *           texture is taken at: the checker and the noise are the reference's within the limits
 *           stated at rt_world_texture_*, and deterministic beyond them
 *
 * Any. RT_QUERY_ANY answers "RT_QUERY_CLOSEST with the same ray would report a hit", the medium's
 * keyed draw included: occluded[i] = 1 or 0. The walk stops at the first test that accepts.
 *
 * Invalid rays. A ray is not walked, its record is t = NaN, flags = RT_HIT_INVALID and zeros
 * (prim, inner, mat = -1; the key echoed), its albedo zeros and its occluded byte 0, when
 *   - a component of o or d, or time, is not finite, or d is (0, 0, 0);
 *   - t_min or t_max is NaN, or t_min > t_max;
 *   - the scene holds a moving sphere and time is outside the scene's [time_lo, time_hi]
 *     (rt_scene_soa: the node boxes bound the spheres for those times only);
 *   - |o| has a component beyond the bound the launch was planned with (below).
 * A few compares per ray before anything is walked; no other ray is affected.
 *
 * Slab tests. The conservative f32 node tests (rt_ctx_set_variant) hold while ray origins stay
 * within 2 * rt_scene_soa.pad_extent. Host-pointer calls take the largest |o component| of the valid
 * rays themselves and plan with it: they flag no ray for its origin. Device-pointer calls plan with
 * origin_bound, and flag every ray with an |o component| beyond it; 0 or a non-finite value means
 * unknown: f64 node tests, no ray flagged for its origin. The f32 node tests also need the ray's
 * largest |d component| within [2^-40, 2^40] (they hold 1/d in f32): a host-pointer call with a
 * valid ray outside takes the f64 tests; a device-pointer call planned with f32 tests flags such a
 * ray. rt_query_stats.slab32 says which tests ran; the bits do not depend on it.
 *
 * Call errors. A null ctx, params, rays or out; n < 0 or n > 2^31 - 1; a mode other than the two;
 * CLOSEST with hits and albedo both NULL or with occluded set; ANY with occluded NULL or with hits
 * or albedo set; on_device with rays or hits not 16-byte aligned: RT_ERR_INVALID. No uploaded scene:
 * RT_ERR_NO_SCENE. RT_PREC_F32 contexts: RT_ERR_UNSUPPORTED. n = 0 is RT_OK and launches nothing.
 * Host pointers: the call is synchronous, and takes the rays in batches whose device copies (rays
 * and results) stay within RT_OPT_TRACE_BUF_BYTES. on_device: the pointers are device pointers and
 * the call is only enqueued on stream (or the context's stream), like rt_render.
 * The kernel is trace_query (one instantiation per kernel variant and mode, picked as rt_render's),
 * one lane per ray. */
typedef struct rt_ray {            /* 80 B; arrays of them 16-byte aligned on the device */
    double o[3], d[3];             /* origin, direction (not normalised: t is in units of d) */
    double time;                   /* the ray's time (moving spheres) */
    double t_min, t_max;           /* hit_hittables' interval */
    uint32_t key_pixel, key_sample;/* coordinates of the constant medium's keyed draw for this ray */
} rt_ray;

enum { RT_HIT_FRONT = 1, RT_HIT_MEDIUM = 2, RT_HIT_INVALID = 4 };
typedef struct rt_hit {            /* 80 B */
    double t;                      /* +inf: a miss; NaN: RT_HIT_INVALID */
    double p[3], n[3];
    int32_t prim, inner, mat, flags;
    uint32_t key_pixel, key_sample;/* echoed from the ray, so shuffled or tiled results identify themselves */
} rt_hit;

enum { RT_QUERY_CLOSEST = 0, RT_QUERY_ANY = 1 };
typedef struct rt_query_params {
    int64_t n;                     /* rays */
    int32_t mode;                  /* RT_QUERY_* */
    int32_t on_device;             /* 0: host pointers, synchronous; 1: device pointers, only enqueued on stream */
    uint64_t seed;                 /* the keyed draw's seed (rt_render_params.render_seed's role) */
    uint32_t bounce;               /* the keyed draw's bounce coordinate; 0 = a primary ray's cast */
    double origin_bound;           /* on_device: the caller's bound on |o| components; host pointers: ignored */
    void* stream;
} rt_query_params;
typedef struct rt_query_out {
    rt_hit* hits;                  /* CLOSEST: n records, or NULL */
    double* albedo;                /* CLOSEST: n x 3, or NULL */
    uint8_t* occluded;             /* ANY: n bytes */
} rt_query_out;
int rt_trace_rays(rt_ctx* ctx, const rt_query_params* p, const rt_ray* rays, const rt_query_out* out);

typedef struct rt_query_stats {
    double kernel_ms;              /* last rt_trace_rays: its trace_query launches (HIP events; waits for them
                                      if the call was only enqueued) */
    int64_t rays;
    int64_t invalid;               /* host-pointer calls: records flagged RT_HIT_INVALID (ANY: rays the host's
                                      own statement of the rules above flags); device-pointer calls: -1 */
    int32_t variant_features;      /* the kernel variant's feature set, as rt_stats.variant_features */
    int32_t slab32;                /* 1: the launches tested f32 node slabs */
    int32_t mode, batches;         /* RT_QUERY_*; launches the call took */
} rt_query_stats;
int rt_query_last_stats(rt_ctx* ctx, rt_query_stats* out);

/* The ray rt_render shoots for every pixel's sample `sample` under render_seed (Camera::get_ray,
 * camera.rs:58-66, after main.rs:517-518's jitter: the path stream of (pixel, sample), its two jitter
 * draws, random_in_unit_disk's tries, the time draw), host code with no context: out[i] has that
 * origin, direction and time, t_min = 0.001, t_max = +inf and the key (y * width + x, sample).
 * tiled = 0: ray i is pixel i (row 0 at the bottom). tiled = 1: 8x8 tiles in tile-grid order,
 * row-major inside a tile, pixels past the image left out (the lane order of the chunk kernels);
 * still width * height records. width, height >= 2, width * height <= 2^31 - 1, sample >= 0. */
int rt_camera_rays(const rt_camera* cam, int width, int height, uint64_t render_seed, int sample, int tiled,
                   rt_ray* out);

/* ---- output ------------------------------------------------------------------------------ */
/* P3 PPM byte for byte as the reference writes it (write_color, math.rs:119-132; main.rs:472,
 * 591-596): header "P3\nW H\n255\n\n", rows top to bottom, each channel
 * (int)(256 * clamp(sqrt(x * (1.0 / samples_per_pixel)), 0, 0.999)) in f64, with Rust's
 * saturating `as i32` (NaN -> 0). rgb is height x width x 3 f64 with row 0 = bottom (y = 0):
 * per-pixel sums over samples_per_pixel samples (rt_accum_get), or rt_render's RT_OUT_F64 mean
 * (already sum * (1/spp)) with samples_per_pixel = 1 — x * 1.0 == x, so both give the
 * reference's bytes. */
int rt_write_ppm_f64(const double* rgb, int samples_per_pixel, int width, int height, const char* path);
/* The same channel values without the file: out[i] for the 3n channels of n pixels, in memory order. */
int rt_write_color(const double* rgb, int samples_per_pixel, int64_t n, int32_t* out);
/* The f32 frame's writer (RT_OUT_F32 output, the f32 mode): as rt_write_ppm_f64 with spp = 1, but
 * the mean was rounded to f32 before the sqrt, so a channel whose 256*sqrt(mean) lies within
 * ~1e-5 of an integer can differ by one from the reference's f64 write_color. */
int rt_write_ppm(const float* mean_rgb, int width, int height, const char* path);

/* Kernel variant knobs of a context: slab32 (conservative f32 BVH slab tests),
 * lds_stack (traversal stack in LDS instead of scratch), lds_nodes (keep the TLAS in LDS
 * when it fits). Defaults 1/1/1. Results do not depend on them (tests check this). */
int rt_ctx_set_variant(rt_ctx* ctx, int slab32, int lds_stack, int lds_nodes);

/* Context options (rt_ctx_set_option / rt_ctx_get_option). The library reads no environment
 * variable: every behaviour switch is one of these or a setter above. Images do not depend on
 * any of them (the tests check this); they trade speed and memory.
 *   RT_OPT_TRACE_BUF_BYTES  bound of the trace-output buffer (below, default 64 GiB); 0 restores the default
 *   RT_OPT_BATCH_OVERLAP    1 (default): buffer batches overlap on two streams; 0: one buffer, in order
 *   RT_OPT_BLOCK_SAMPLES    per-sample pool: samples per work block (0: auto, 16 down to 4 for small shards)
 *   RT_OPT_BLOCK_CHUNKS     item pool: chunks per work block (0: auto = 2)
 *   RT_OPT_EXTRA_FEATURES   feature bits OR-ed into the scene's, so a scene runs on a larger
 *                           feature-set variant than it needs (tests: the all-features variant)
 *   RT_OPT_HOIST            1 (default): the spheres variants test a huge root-child leaf before
 *                           the walk (SceneDev.pre_leaf); takes effect at the next upload
 *   RT_OPT_POOL_RING        1 (default): POOL reduces each finished (tile, chunk) block inside the
 *                           trace kernel into chunk partials when its per-sample buffer would not
 *                           fit the bound in one batch; 2: whenever its blocks allow; 0: never (the
 *                           per-sample buffer and reduce_samples; see RT_SCHED_POOL)
 *   RT_OPT_COMM_DIRECT      1 (default): rt_render_gather on a communicator of one rank, with the
 *                           context in raster tile order, is rt_render straight into the frame (a
 *                           world of one has nothing to gather); 0: the tile shard, the RCCL gather
 *                           and the reorder kernel as at any other world size (tests)
 *   RT_OPT_AUTO_DEAL_ORDER  1 (default): whole-frame pool renders are dealt in the cost order the
 *                           render itself measured (rt_last_deal_order); 0: raster order, nothing
 *                           measured; 2: every render measures, none is reordered (A/B runs)
 *   RT_OPT_PRIMARY_CANDIDATES  1 (default): a new sample of the f64 spheres variant's per-sample pool
 *                           takes its first hit from an exact test of its pixel's candidate primitives (a
 *                           table built once per scene upload, camera and frame size inside the render, 16 B
 *                           per pixel, skipped above 256 MiB) and joins the walk with its first bounce ray;
 *                           0: every primary ray walks. Same bits either way.
 *   RT_OPT_PRIMARY_CANDIDATES_K  candidates a pixel's record may hold before the pixel is flagged
 *                           "walk" (1..7, default 7; tests force 1); takes effect at the next table build
 *   RT_OPT_SKIP_SKY_TILES   1 (default): a whole-frame rt_render through the per-sample buffer that has a
 *                           primary-candidate table and a deal table (RT_OPT_AUTO_DEAL_ORDER 1 or 2),
 *                           at max_depth >= 1, traces no 8x8 tile whose pixels' candidate lists are all
 *                           empty: each of their samples is exactly the background, and the reduction
 *                           sums that constant as it would have summed the records (rt_stats.sky_tiles).
 *                           0: every tile is traced. Same bits either way.
 *   RT_OPT_DEFER_ROOTS      1 (default): where the primary-candidate kernel runs (RT_OPT_PRIMARY_CANDIDATES), its
 *                           sphere tests decide "near or far root, in range, closer than the best" from f32
 *                           brackets of the roots with a proven bound, fall back to the exact root where a
 *                           bracket cannot decide, and compute the exact f64 root of a cast's closest sphere
 *                           only (rt_stats.defer_roots); 0: every candidate's exact root, as before. Same bits
 *                           either way. */
enum {
    RT_OPT_TRACE_BUF_BYTES = 1,
    RT_OPT_BATCH_OVERLAP = 2,
    RT_OPT_BLOCK_SAMPLES = 3,
    RT_OPT_BLOCK_CHUNKS = 4,
    RT_OPT_EXTRA_FEATURES = 5,
    RT_OPT_HOIST = 6,
    /* 7, 8: ABI v4's wavefront-schedule options, removed with it (RT_ERR_INVALID) */
    RT_OPT_POOL_RING = 9,
    RT_OPT_COMM_DIRECT = 10,
    RT_OPT_AUTO_DEAL_ORDER = 11,
    RT_OPT_PRIMARY_CANDIDATES = 12,
    RT_OPT_PRIMARY_CANDIDATES_K = 13,
    RT_OPT_SKIP_SKY_TILES = 14,
    RT_OPT_DEFER_ROOTS = 15
};
int rt_ctx_set_option(rt_ctx* ctx, int key, int64_t value);
int rt_ctx_get_option(rt_ctx* ctx, int key, int64_t* value);

/* Work schedule of a context (default RT_SCHED_AUTO). In RT_PREC_F64 images are bit-identical
 * under all of them; in RT_PREC_F32 each schedule's kernel rounds on its own (rt_ctx_set_precision).
 *   CHUNKS: a wave owns an 8x8 tile x one chunk of samples, each lane one pixel's chunk,
 *           written as one partial per (pixel, chunk); the wave waits for its slowest lane.
 *   POOL:   persistent waves take (tile, chunk) blocks from a device counter and a lane
 *           whose path ended takes the block's next (pixel, sample) at once. Every sample's
 *           radiance goes to a per-sample buffer ([8x8 tile][sample][pixel of the tile]) summed
 *           per pixel in sample order by a second kernel. When that buffer does not fit the bound
 *           in one batch (RT_OPT_POOL_RING), a block belongs to one wave instead: its samples wait
 *           in that wave's ring of 4 blocks, and when the block's last sample ends the wave sums
 *           every pixel's samples in order into the chunk partial (1/chunk of the per-sample
 *           bytes, as ITEMS). Same bits either way in RT_PREC_F64 (in RT_PREC_F32 the ring form is
 *           another kernel: other last bits).
 *   ITEMS:  persistent waves as POOL, but a lane takes a whole (pixel, chunk) item, traces
 *           its samples in order and writes one partial, as CHUNKS does (1/chunk of POOL's
 *           buffer bytes); a lane whose item ended takes the next item at once.
 *   AUTO:   ITEMS for the Cornell-box variant (rects, boxes and instances without media: measured
 *           fastest there); otherwise POOL when it can reduce in the kernel or its
 *           per-sample radiance is at most 4 x the buffer bound, else ITEMS; rt_stats.schedule
 *           reports which ran.
 * Schedule 4 (ABI v4's wavefront split: wf_logic / wf_trace kernels over a path pool in HBM) was
 * measured 2.3x slower than POOL on the final scene and removed; rt_ctx_set_schedule(4) returns
 * RT_ERR_UNSUPPORTED (the code: scripts/experiments/r05_wavefront.patch).
 * The trace-output buffer (POOL's ring included) is bounded by RT_OPT_TRACE_BUF_BYTES (default
 * 64 GiB, or half the device's free memory if that is less; allocated lazily, as large as a
 * render needs). A larger render runs in buffer
 * batches whose sums are carried across, in two halves of the bound: batch k traces into half
 * k & 1 on one of two context streams while the render's stream reduces batch k - 1, so
 * consecutive traces overlap (RT_OPT_BATCH_OVERLAP 0: one buffer, in order). Under the default
 * bound C2 (11.5 GB) and C4 (49.8 GB) render through the per-sample buffer in one batch, C5
 * (1.6 TB of records) through the ring's chunk partials in a few. */
enum { RT_SCHED_CHUNKS = 0, RT_SCHED_POOL = 1, RT_SCHED_ITEMS = 2, RT_SCHED_AUTO = 3 };
int rt_ctx_set_schedule(rt_ctx* ctx, int schedule);

/* Arithmetic of a context's renders (default RT_PREC_F64).
 *   F64: the reference's f64 everywhere (math.rs:13-17), path-identical to the oracle: the
 *        same rays, hits and draws; the per-pixel means differ only in the last ulps (the
 *        throughput product T = a0*a1*...*e associates left here, right in the recursive
 *        ray_color, main.rs:31; L_inf ~3e-16 at full C2 spp). Exact-t ties between two
 *        primitives resolve by test order, which a BVH (and the hoisted root leaf) changes
 *        against the reference's list order — a measure-zero event for spheres.
 *   F32: a fast mode: f32 rays, hit records, materials and textures (sphere tests keep
 *        |oc|^2 - r^2 in f64), one 32-bit draw per uniform; per-pixel sums
 *        stay f64. Statistically equal to F64 (independent-seed tests), not bitwise; never
 *        the headline metric. count_work is not available in it. Its translation units
 *        contract multiply-adds, and each trace kernel (CHUNKS, POOL with its buffer, POOL
 *        with its ring, ITEMS) compiles the path code on its own, so an F32 frame depends on
 *        the kernel that ran: rt_stats.schedule, and ring_bytes > 0 or not. For one kernel it
 *        is bit-identical across row and tile shards, world sizes, tile orders, deal orders and
 *        buffer batches, as every F64 frame is across all of these and across kernels too. */
enum { RT_PREC_F64 = 0, RT_PREC_F32 = 1 };
int rt_ctx_set_precision(rt_ctx* ctx, int precision);

/* ---- self test ------------------------------------------------------------------------------ */
/* Evaluates rt_numerics.h functions on the device (same fn ids as the oracle's
 * orc_eval) so tests can check host/device bit equality. */
int rt_device_eval(rt_ctx* ctx, int fn, const double* x, const double* y, const double* z, double* out, int n);

#ifdef __cplusplus
}
#endif
#endif
