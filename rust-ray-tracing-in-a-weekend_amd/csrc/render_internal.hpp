// render_internal.hpp — what the auxiliary passes (abi_passes.cpp) need of the render driver
// (abi.cpp): where a sample range's sums go, the launch params of a range, and the driver
// itself. Private to the library, as ctx_internal.hpp is.
#pragma once

#include "ctx_internal.hpp"
#include "launch_plan.hpp"
#include "trace_kernel.hpp"

#pragma GCC visibility push(hidden)

using rtp::auto_chunk;
using rtp::bad_geometry;
using rtp::Layout;
using rtp::layout_of;
using rtp::row_block_of;

// device slots for launch params (a ring: a render's params stay intact while later
// renders are enqueued behind it on the same stream)
constexpr int kParamSlots = 16;

// Where a sample range's per-pixel sums go: added to acc (n_px x 3 f64), or (acc null)
// written as sum * scale to out (f32 / f64).
struct Sink {
    double* acc = nullptr;
    void* out = nullptr;
    bool f64 = true;
    double scale = 1.0;
    // rt_render_adaptive's passes (acc and out unused): a tile shard under the call's own tile
    // order (moments->order), on the per-sample buffer whatever the context's schedule, reduced by
    // the moments kernel into the call's frame-layout accumulators; n_done = samples per pixel
    // of the shard's tiles once this range is in
    const rtk::AdaptiveFrame* moments = nullptr;
    int n_done = 0;
    const rtk::AdaptiveHalves* halves = nullptr;   // rt_render_adaptive_halves: the half sums beside them
};

// What a plan launches: the scene's device view with the plan's staged counts, and the launch
// options (timed: a count_work render sets o.count)
struct PlannedLaunch {
    rtk::SceneDev S;
    rtk::LaunchOpts o;
};
inline PlannedLaunch planned_launch(const rtk::SceneDev& scene, const rtp::Plan& pl)
{
    PlannedLaunch l{scene, {}};
    l.S.n_lds_nodes = pl.n_lds_nodes;
    l.S.n_lds_materials = pl.n_lds_materials;
    l.S.n_lds_textures = pl.n_lds_textures;
    l.S.n_lds_blas = pl.n_lds_blas;
    l.S.seed_stage_bytes = (int32_t)pl.seed_stage_bytes;
    l.o.features = pl.features;
    l.o.slab32 = pl.slab32;
    l.o.lds_stack = pl.lds_stack;
    l.o.count = 0;
    l.o.pool = pl.schedule;
    l.o.f32 = pl.f32;
    return l;
}

// The launch params of a sample range, all but what the plan and the batch loop set (block sizes,
// ring, sample range, work blocks). Fails on a context tile order that is not the frame's.
int fill_kparams(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const Layout& lay, int chunk,
                 const Sink& sink, int64_t img_tiles, rtk::KParams& K);

// Traces samples [s_begin, s_end) of the shard in chunks of `chunk` and reduces them into the
// sink (abi.cpp); the render span's events bracket the trace launches and the reductions.
int run_range(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int s_begin, int s_end, int chunk,
              hipStream_t stream, const Sink& sink);

#pragma GCC visibility pop
