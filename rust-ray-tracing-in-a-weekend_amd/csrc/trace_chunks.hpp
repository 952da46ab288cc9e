// trace_chunks.hpp — the chunk schedule (the first schedule of trace_device.hpp, kept for A/B): a
// lane traces one pixel's chunk of samples and writes their sum as one partial, [chunk][pixel].
#pragma once
#include "trace_shade.hpp"
#include "trace_grid.hpp"

namespace rtk {

// KParams comes by pointer: read where used (scalar loads) instead of pinning ~70 SGPRs
// for the whole kernel (by value it spilled SGPRs into VGPR lanes).
template <class C>
__global__ void __launch_bounds__(BlockThreads<C>(), min_waves<C>()) trace_chunks(SceneDev S, const KParams* __restrict__ Pp,
                                                                    double* __restrict__ partial,
                                                                    unsigned long long* __restrict__ counters)
{
    const KParams& P = *Pp;
    stage_lds<C>(S);   // every thread of the block takes part, before any early return
    LaneWork w;
    if (!lane_work(P, w)) return;
    StackT<C> stack;
    if constexpr (Stack16Cfg<C>()) stack.base = reinterpret_cast<short*>(rt_lds + lds_stack_offset<C>(S)) + threadIdx.x;
    else if constexpr (C::LDS) stack.init((int)lds_stack_offset<C>(S));
    Count cnt{};
    uint64_t t_cam = 0, t_trace = 0, t_shade = 0, t_prev = 0;
    if (C::COUNT) t_prev = __builtin_amdgcn_s_memtime();
    using R = typename C::Real;
    double sum_r = 0.0, sum_g = 0.0, sum_b = 0.0;
    Keyed key{P.seed, w.pixel, 0, 0};
    rt_pstream st;
    RayT<R> r;
    R Tr = 1, Tg = 1, Tb = 1;
    int depth = 0;
    int s = w.s_begin;
    bool new_sample = true;
    while (s < w.s_end) {
        if (C::COUNT && first_active_lane()) cnt.wave_steps++;
        if (new_sample) {
            new_sample = false;
            if constexpr (C::F32) ds_start_f32(st, P.seed, w.pixel, (uint32_t)s);
            else ds_start(st, P.seed, w.pixel, (uint32_t)s);
            key.sample = (uint32_t)s;
            camera_ray(P, w.ix, w.y, st, r);
            finish_ray<C>(r, S.has_spheres != 0);
            Tr = Tg = Tb = (R)1;
            depth = P.max_depth;
        }
        if (C::COUNT) { const uint64_t t = __builtin_amdgcn_s_memtime(); t_cam += t - t_prev; t_prev = t; }
        bool cont = false;
        if (depth > 0) {  // main.rs:21-23: depth 0 is black
            key.bounce = (uint32_t)(P.max_depth - depth);
            if (C::COUNT) cnt.casts++;
            HitT<R> h;
            const bool hit = trace_world<C>(S, r, h, stack, key, cnt);
            if (C::COUNT) { const uint64_t t = __builtin_amdgcn_s_memtime(); t_trace += t - t_prev; t_prev = t; }
            if (!hit) {  // main.rs:37: background
                sum_r = sum_r + Tr * P.bg[0];
                sum_g = sum_g + Tg * P.bg[1];
                sum_b = sum_b + Tb * P.bg[2];
            } else {
                cont = shade<C>(S, P, h, r, st, Tr, Tg, Tb, sum_r, sum_g, sum_b);
            }
        }
        if (C::COUNT) { const uint64_t t = __builtin_amdgcn_s_memtime(); t_shade += t - t_prev; t_prev = t; }
        if (cont) {
            depth -= 1;
        } else {
            s += 1;
            new_sample = true;
        }
    }
    double* o = partial + (((size_t)w.chunk * P.n_rows + w.k) * P.width + w.x) * 3;
    o[0] = sum_r;
    o[1] = sum_g;
    o[2] = sum_b;
    if (C::COUNT) {
        atomicAdd(&counters[kCtrCasts], (unsigned long long)cnt.casts);
        atomicAdd(&counters[kCtrNodeVisits], (unsigned long long)cnt.nodes);
        atomicAdd(&counters[kCtrPrimTests], (unsigned long long)cnt.prims);
        atomicAdd(&counters[kCtrWaveSteps], (unsigned long long)cnt.wave_steps);
        atomicAdd(&counters[kCtrWaveNodeSteps], (unsigned long long)cnt.wave_nodes);
        atomicAdd(&counters[kCtrWaveLeafSteps], (unsigned long long)cnt.wave_leaves);
        atomicAdd(&counters[kCtrCameraLanes], (unsigned long long)cnt.cam_lanes);
        atomicAdd(&counters[kCtrCameraSteps], (unsigned long long)cnt.cam_steps);
        atomicAdd(&counters[kCtrShadeLanes], (unsigned long long)cnt.shade_lanes);
        atomicAdd(&counters[kCtrShadeSteps], (unsigned long long)cnt.shade_steps);
        // phase times are per wave (every active lane sees the same clock): one lane adds
        if ((int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1) {
            atomicAdd(&counters[kCtrCyclesCamera], (unsigned long long)(t_cam + cnt.t_seed + cnt.t_tries));   // ray generation, all of it
            atomicAdd(&counters[kCtrCyclesSeed], (unsigned long long)cnt.t_seed);
            atomicAdd(&counters[kCtrCyclesTries], (unsigned long long)cnt.t_tries);
            atomicAdd(&counters[kCtrCyclesTrace], (unsigned long long)t_trace);
            atomicAdd(&counters[kCtrCyclesShade], (unsigned long long)t_shade);
            atomicAdd(&counters[kCtrCyclesNodes], (unsigned long long)cnt.t_nodes);
            atomicAdd(&counters[kCtrCyclesLeaves], (unsigned long long)cnt.t_leaves);
        }
    }
}

}  // namespace rtk
