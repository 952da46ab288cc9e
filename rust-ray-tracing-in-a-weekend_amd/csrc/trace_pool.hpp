// trace_pool.hpp — the pool schedules (the default schedules of trace_device.hpp): persistent waves
// that take work blocks from a device counter and whose lanes take a block's next unit as their
// paths end; the per-sample pool's record ring and its in-kernel reduction, the deal order of a
// whole frame, the wave-wide sample starts, and the trace_pool kernel.
#pragma once
#include "trace_shade.hpp"
#include "trace_grid.hpp"

namespace rtk {

// ---------------------------------------------------------------------------
// Sample-pool schedule. Persistent waves take work blocks (one 8x8 tile x one chunk of
// samples) from a global counter; inside the wave, a lane whose path ended takes the
// block's next (pixel, sample) unit at once (ballot + mbcnt), so lanes do not idle until
// the last blocks run out. Each sample's radiance goes to its own slot of a buffer
// ([tile][sample][pixel of the tile], tiled_record); reduce_samples_tiled then sums every pixel's samples in sample order,
// so the image does not depend on which lane or wave computed a sample.
// ---------------------------------------------------------------------------
// The hit record's old contents are dead: freeze(poison) for every field, so the
// register allocator need not carry them through the walk that writes the next record.
template <class R>
__device__ __forceinline__ void forget(HitT<R>& h)
{
    h.t = __builtin_nondeterministic_value(h.t);
    h.px = __builtin_nondeterministic_value(h.px);
    h.py = __builtin_nondeterministic_value(h.py);
    h.pz = __builtin_nondeterministic_value(h.pz);
    h.nx = __builtin_nondeterministic_value(h.nx);
    h.ny = __builtin_nondeterministic_value(h.ny);
    h.nz = __builtin_nondeterministic_value(h.nz);
    h.uv0 = __builtin_nondeterministic_value(h.uv0);
    h.uv1 = __builtin_nondeterministic_value(h.uv1);
    h.uv2 = __builtin_nondeterministic_value(h.uv2);
    h.uv3 = __builtin_nondeterministic_value(h.uv3);
    h.front = __builtin_nondeterministic_value(h.front);
    h.mat = __builtin_nondeterministic_value(h.mat);
    h.uvkind = __builtin_nondeterministic_value(h.uvkind);
}

__device__ __forceinline__ unsigned lanes_below(uint64_t mask)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Per-sample pool, in-kernel reduction (kPoolRing): the whole wave sums one finished block —
// lane p the tile's pixel p — over its samples in order from 0.0, reduce_samples_tiled's chunk sum,
// and writes the chunk partial ([chunk][pixel], reduce_chunks' input). The block is one chunk
// of samples (block_samples == spp_chunk, chunk-aligned batches), so the chunk is its group.
#ifndef RING_LOADS
#define RING_LOADS 4
#endif
// lane q of v set to val (the ring state's writes; readlane reads it back as a scalar)
__device__ __forceinline__ int ring_set(int val, int q, int v) { return (int)__lane_id() == q ? val : v; }

template <class C>
__device__ __forceinline__ double* ring_of_wave(const KParams& P)
{
    const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (unsigned)(BlockThreads<C>() / 64) + threadIdx.x / 64u);
    return P.ring + (size_t)wave * kRingWaveDoubles;
}
// the ring's header after the records: the block id of each slot (RingSgpr variants)
__device__ __forceinline__ unsigned* ring_block_id(double* ring_wave)
{
    return reinterpret_cast<unsigned*>(ring_wave + (size_t)kPoolRing * kRingSlot * 3);
}
// Where a wave tracks its blocks in flight. The spheres variant: the occupied slots and the
// current slot in SGPRs, the block ids in the ring's header (C2 1200x800x500 73.92 ms against
// 74.45 with the VGPR below; round 4's per-sample buffer 74.52). The others (the final variant's
// SGPRs are at the limit; there the SGPR form took C4 1920x1080x256 to 269.2 ms against 266.9):
// the lanes of one VGPR (profiles/r05o_ab_c{2,4}.log).
template <class C>
constexpr bool RingSgpr() { return C::F == FEAT_SET_SPHERES; }
// Which pool kernels carry a whole frame's deal order and the block-cost measurement behind it
// (KParams.tile_major = kDealOrdered / kDealMeasure, the table at kDealTable; deal_cache.hpp).
template <class C>
constexpr bool DealCfg() { return deal_variant(C::F) && !C::COUNT; }

// Wave-wide sample starts (launch_shapes.hpp, RT_STAGE_SEEDS; the per-sample pool's CfgStage
// instantiations). A slot is what a lane needs to start its sample in the `cam_wait` state: the
// path stream after the two jitter draws, and the jitter. Slot j of the workgroup's area belongs
// to lane j % 64 of wave j / 64, so the writer's index is threadIdx.x.
struct alignas(32) SeedSlot {
    rt_pstream st;
    double u, v;
};
static_assert(sizeof(SeedSlot) == kSeedSlotBytes, "a staged sample start is one slot");
template <class C, bool ITEMS>
constexpr bool StagedPool()   // trace_pool<C, ITEMS, ...> stages: the f64 spheres variant's 16-bit-stack per-sample pool kernels
{
    static_assert(!C::STAGE || (Stack16Cfg<C>() && RingSgpr<C>() && !C::F32), "staged sample starts: the f64 spheres variant's 16-bit-stack kernels");
    return C::STAGE && !ITEMS;
}
template <class C>
__device__ __forceinline__ SeedSlot* seed_slots(const SceneDev& S)   // derived where used, like lds_stack_offset: nothing of it lives through the walk
{
    return reinterpret_cast<SeedSlot*>(reinterpret_cast<char*>(rt_lds) + lds_seeds_offset(lds_layout_of<C>(S).total));
}

__device__ __forceinline__ void ring_reduce(const KParams& P, const double* __restrict__ rec,
                                            double* __restrict__ partial, unsigned blk, unsigned n_tiles, unsigned group,
                                            size_t n_px, int lane)
{
    // the block's (sample group, tile), as trace_pool dealt it (KParams.deal_div)
    const unsigned outer = blk / P.deal_div, inner = blk - outer * P.deal_div;
    const unsigned grp = P.tile_major ? inner : outer, tile = P.tile_major ? outer : inner;
    const int s0 = P.sample_begin + (int)(grp * group);
    const int x = (int)(tile % (unsigned)P.tiles_x) * 8 + (lane & 7);
    const int k = (int)(tile / (unsigned)P.tiles_x) * 8 + (lane >> 3);
    const int ns = min(P.spp, s0 + (int)group) - s0;
    // the records were stored by lanes of this wave: order their stores before these loads
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    // one channel at a time, RING_LOADS samples' loads in flight (the wave's path state stays live
    // beside them; one load per round trip left the wave waiting on L2 ~48 times per block)
    constexpr int NB = RING_LOADS;
    const bool own = x < P.width && k < P.n_rows;
    double* o = partial + ((size_t)grp * n_px + (size_t)k * P.width + x) * 3;
#pragma unroll 1
    for (int c = 0; c < 3; ++c) {
        const double* p = rec + (size_t)lane * 3 + c;
        double a = 0.0;
#pragma unroll 1
        for (int j0 = 0; j0 < ns; j0 += NB) {
            double v[NB];
#pragma unroll
            for (int j = 0; j < NB; ++j) v[j] = j0 + j < ns ? p[(size_t)j * 64 * 3] : 0.0;
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if (j0 + j < ns) a = a + v[j];
            p += (size_t)NB * 64 * 3;
        }
        if (own) o[c] = a;
    }
}

// New samples resolved from per-pixel candidate lists (CfgPrimary; primary_candidates.hpp, DESIGN.md
// §5.2). Every primary ray of a pixel lies in a thin double cone, and the primitives that cone can
// touch are a handful, known per (scene, camera, frame size): KParams.primary holds them per image
// pixel. A new sample whose pixel is listed takes its closest hit from an exact test of those
// candidates — the walk's own simple_t and finish_hit, t_max updated as do_leaf does; the closest
// hit does not depend on the order of the tests — scatters, and joins the walk with its first
// bounce ray in the same iteration, so a sample holds its lane for one iteration fewer. A flagged
// pixel's sample (or any at max_depth 0) walks as before. Ray generation in two rejection loops,
// each under the RT_TRY_LEFT rule: the new samples' disk tries, then the scatter tries of every
// pending lane, those of this iteration's primary hits included. Each lane's draws keep their order.
template <class C, bool ITEMS>
constexpr bool PrimaryPool()
{
    static_assert(!C::PRIMARY || (C::STAGE && !C::COUNT && C::F == FEAT_SET_SPHERES && TryLeft<C>()),
                  "primary candidates: the f64 spheres variant's timed staged kernels");
    return C::PRIMARY && StagedPool<C, ITEMS>();
}
template <class C, class R = typename C::Real>
__device__ __forceinline__ void generate_primary(const SceneDev& S, const KParams& P, int x, int k, int& depth, bool& new_sample,
                                                 bool& pending, rt_pstream& st, RayT<R>& r, HitT<R>& h, R& Tr, R& Tg, R& Tb,
                                                 double& cr, double& cg, double& cb, bool& go, bool& gen_wait, Count& cnt)
{
    go = false;
    if (__any(new_sample)) {   // (wave-uniform)
        uint4 rec = make_uint4(0xffffu, 0u, 0u, 0u);
        if (new_sample) {
            int ix, y;
            image_xy(P, x, k, ix, y);
            // (a tile shard's grid is whole 8x8 tiles: an edge tile's lanes beyond the frame have no
            // record, and walk)
            if ((unsigned)ix < (unsigned)P.img_width && (unsigned)y < (unsigned)P.height)
                rec = P.primary[(size_t)y * (size_t)P.img_width + (size_t)ix];
        }
        R qx = (R)0, qy = (R)0, qz = (R)0, l2 = (R)1;
        bool accepted = !new_sample;
        for (int n = 1;; ++n) {
            if (!accepted) accepted = unit_try(st, (R)P.scale_m11, false, qx, qy, qz, l2);
            const uint64_t rejecting = __ballot(!accepted);
            if (rejecting == 0 || (n >= RT_TRY_MIN && __popcll(rejecting) <= RT_TRY_LEFT)) break;
        }
        // the candidates of the lanes whose camera ray is ready and whose pixel is listed
        unsigned n_cand = 0;
        if (new_sample && !accepted) {
            gen_wait = true;   // the jitter stays in r.dx / r.dy, the tries go on in the next iteration
        } else if (new_sample) {
            new_sample = false;
            const R u = r.dx, v = r.dy;
            camera_end(P, st, u, v, qx, qy, r);
            const unsigned n = rec.x & 0xffffu;
            if (n > 7u || depth <= 0) go = true;   // a flagged pixel (0xffff; or depth 0: black, as before): today's path
            else {
                finish_ray<C, false>(r, true);   // the sphere part: |d|^2 and its reciprocal
                n_cand = n + 1;                  // (+ 1: a listed lane with no candidate still ends its sample below)
            }
        }
        if (__any(n_cand != 0)) {
            const R t_min = (R)0.001;
            R t_max = (R)RT_INF;
            HitRefT<R> best;
            best.sub = 0;
            best.side = 0;
            best.prim = -1;
            [[maybe_unused]] rtrb::Best bb = rtrb::none();   // CfgDefer: the slot and an f32 bracket of its t (root_bracket.hpp)
            // the record's slots (halfwords 1..7) in order: three from the first pair of words, then four
            uint64_t a = ((uint64_t)rec.y << 32 | (uint64_t)rec.x) >> 16;
            const uint64_t b = (uint64_t)rec.w << 32 | (uint64_t)rec.z;
            // as many passes as the longest list among these lanes (wave-uniform: a ballot of the active lanes)
#pragma unroll 1
            for (unsigned i = 0; __ballot(i + 1 < n_cand) != 0; ++i) {
                if (i + 1 < n_cand) {
                    const int slot = (int)((unsigned)a & 0xffffu);
                    if constexpr (C::DEFER) {
                        (void)sphere_defer_t<C>(S, r, rtrb::ya32(r.ya), slot, t_min, bb);
                    } else if (simple_t<C>(S.leaf_prims[slot], r, t_min, t_max, best.t, best.side, cnt, false)) {
                        best.prim = slot;
                        t_max = best.t;
                    }
                }
                a >>= 16;
                if (i == 2) a = b;
            }
            if constexpr (C::DEFER) best.prim = bb.prim;
            if (n_cand != 0) {
                if (best.prim < 0) {   // main.rs:37: background; the sample ends
                    cr = cr + Tr * P.bg[0];
                    cg = cg + Tg * P.bg[1];
                    cb = cb + Tb * P.bg[2];
                } else {
                    if constexpr (C::DEFER) (void)sphere_exact_of<C>(S, r, best.prim, t_min, best.t);   // the winner's exact root, once
                    finish_hit<C>(S, r, best, h);
                    pending = shade_begin<C>(S, h, Tr, Tg, Tb, cr, cg, cb);
                }
            }
        }
    }
    // the scattered rays of the pending lanes, as the merged loop draws them
    if (__any(pending)) {
        R qx = (R)0, qy = (R)0, qz = (R)0, l2 = (R)1;
        bool accepted = !(pending && shade_draws<C>(S, h.mat));
        for (int n = 1;; ++n) {
            if (!accepted) accepted = unit_try(st, (R)P.scale_m11, true, qx, qy, qz, l2);
            const uint64_t rejecting = __ballot(!accepted);
            if (rejecting == 0 || (n >= RT_TRY_MIN && __popcll(rejecting) <= RT_TRY_LEFT)) break;
        }
        if (pending) {
            if (!accepted) {
                gen_wait = true;
            } else {
                pending = false;
                go = shade_end<C, false>(S, h, r, st, Tr, Tg, Tb, qx, qy, qz, l2);
                if (go) depth -= 1;
            }
        }
    }
}

// ITEMS (the item pool, default): a unit is a (pixel, chunk) item instead of one sample.
// The lane that takes it traces the chunk's samples in order, summing their radiance in
// registers exactly as trace_chunks does, and writes one partial per (pixel, chunk) when
// the last one ends; a lane whose item ended takes the next item at once, as in the
// per-sample pool, so lanes still do not idle. Output: chunk partials for
// reduce_chunks, 1/chunk of the per-sample buffer's bytes.
template <class C, bool ITEMS, bool RING = false>
__global__ void __launch_bounds__(BlockThreads<C>(), min_waves<C>()) trace_pool(SceneDev S, const KParams* __restrict__ Pp,
                                                                  double* __restrict__ samples,
                                                                  unsigned long long* __restrict__ counters,
                                                                  unsigned* __restrict__ work)
{
    const KParams& P = *Pp;
    stage_lds<C>(S);
    StackT<C> stack;
    if constexpr (Stack16Cfg<C>()) stack.base = reinterpret_cast<short*>(rt_lds + lds_stack_offset<C>(S)) + threadIdx.x;
    else if constexpr (C::LDS) stack.init((int)lds_stack_offset<C>(S));
    Count cnt{};
    uint64_t t_cam = 0, t_trace = 0, t_shade = 0, t_prev = 0, t_start = 0, t_sample = 0;
    if (C::COUNT) t_prev = t_start = __builtin_amdgcn_s_memtime();
    (void)t_trace;
    (void)t_start;
    (void)t_sample;
    const int lane = threadIdx.x & 63;
    const unsigned n_tiles = (unsigned)P.tiles_x * (unsigned)P.tiles_y;
    // a work block = one tile x block_chunks consecutive chunks (items chunk-major; the
    // per-sample pool's units sample-major): lanes stay on one tile longer, and its rays
    // are coherent (C2 item pool, chunks of 4: 108.4 ms with blocks of one chunk, 101.8 with 8)
    // per-sample pool: a block = one tile x block_samples consecutive samples (any count: the
    // per-sample output does not depend on it)
    const unsigned group = ITEMS ? (unsigned)P.block_chunks : (unsigned)P.block_samples;
    const unsigned n_blocks = P.n_work_blocks;   // n_tiles x ceil(samples or chunks / group)
    const size_t n_px = (size_t)P.n_rows * (size_t)P.width;
    // current work block (wave-uniform)
    unsigned blk_units = 0, blk_next = 0, nvalid = 1;
    int tx0 = 0, tk0 = 0, vw = 1, s0 = 0;
    bool exhausted = false;
    // lane state
    bool active = false, new_sample = false;
    int x = 0, k = 0, s = 0, depth = 0;
    int left = 0;      // ITEMS: samples of the lane's item still to trace after the current one
    bool own = false;  // ITEMS: the lane's item has a next sample (taken before any new unit)
    using R = typename C::Real;
    double cr = 0, cg = 0, cb = 0;
    R Tr = 1, Tg = 1, Tb = 1;
    Keyed key{P.seed, 0, 0, 0};
    rt_pstream st;
    RayT<R> r;
    HitT<R> h;             // a hit whose scattered ray the next iteration draws
    bool pending = false;
    bool cam_wait = false;  // RT_TRY_LEFT: camera_begin ran, the disk tries go on (u, v in r.dx, r.dy)
    (void)cam_wait;
    // In-kernel reduction (RING, the per-sample pool with P.ring; kPoolRing): the wave's blocks
    // in flight (RingSgpr: where), wave-uniform — the occupied slots (bit q), the slot units are
    // taken from, each slot's block. A lane's record index in the wave's ring (slot x kRingSlot +
    // sample of the block x 64 + pixel of the tile) rides in the bits of `s` above
    // kRingSampleBits, so a block is finished when it is not the one units are taken from and no
    // active lane holds one of its units.
    constexpr bool ring = RING && !ITEMS;
    // (the two forms are separate `if constexpr` blocks, not else-branches of one another: written
    // as else-branches the spheres variant's kernel compiled to other code, 1.4 % slower on C2)
    int ringv = 0;                       // !RingSgpr: lane q slot q's block, kRingCur, kRingOcc
    unsigned occ = 0, cur_slot = 0;      // RingSgpr (the other form: read from ringv where used)
    // Staged sample starts (StagedPool): when units are taken from the start of a sample row of the
    // block, the wave first seeds and jitters the whole row — lane p the tile's pixel p — into its
    // LDS slots; a lane that takes a unit reads its slot and is then in the `cam_wait` state (the
    // stream past the jitter draws, u and v in r.dx / r.dy), so ray generation holds no seeding
    // code. Everything is derived from blk_next, nvalid, s0, tx0 and tk0: no state of its own, and
    // no local of its own here either (a constant declared at this point changed the ring kernels'
    // register allocation in every variant).
    for (;;) {
        if constexpr (ring && !RingSgpr<C>()) {   // (final variant) the same, the state in ringv's lanes
            unsigned occv = (unsigned)__builtin_amdgcn_readlane(ringv, kRingOcc);
            if (occv != 0) {
                const unsigned open = blk_next < blk_units ? (unsigned)__builtin_amdgcn_readlane(ringv, kRingCur) : 99u;
#pragma unroll
                for (int q = 0; q < kPoolRing; ++q) {
                    if ((occv >> q & 1u) && (unsigned)q != open &&
                        __ballot(active && ((unsigned)s >> kRingSampleBits) / kRingSlot == (unsigned)q) == 0) {
                        ring_reduce(P, ring_of_wave<C>(P) + (size_t)q * kRingSlot * 3, samples,
                                    (unsigned)__builtin_amdgcn_readlane(ringv, q), n_tiles, group, n_px, lane);
                        occv &= ~(1u << q);
                        ringv = ring_set((int)occv, kRingOcc, ringv);
                    }
                }
            }
        }
        if (ring && RingSgpr<C>()) {   // blocks whose last sample ended: every pixel's samples summed in order
            if (occ != 0) {
                const unsigned open = blk_next < blk_units ? cur_slot : 99u;
#pragma unroll
                for (int q = 0; q < kPoolRing; ++q) {
                    if ((occ >> q & 1u) && (unsigned)q != open &&
                        __ballot(active && ((unsigned)s >> kRingSampleBits) / kRingSlot == (unsigned)q) == 0) {
                        double* rw = ring_of_wave<C>(P);
                        ring_reduce(P, rw + (size_t)q * kRingSlot * 3, samples,
                                    (unsigned)__builtin_amdgcn_readfirstlane(ring_block_id(rw)[q]), n_tiles, group, n_px, lane);
                        occ &= ~(1u << q);
                    }
                }
            }
        }
        if (ITEMS && own) {
            own = false;
            active = true;
            new_sample = true;
            s += 1;
            left -= 1;
        }
        uint64_t need = __ballot(!active);
        while (need != 0 && !exhausted) {
            if (blk_next == blk_units) {
                int free_slot = -1;
                if (ring) {   // a free ring slot first: every one holds an unfinished block -> wait
                    if constexpr (!RingSgpr<C>()) occ = (unsigned)__builtin_amdgcn_readlane(ringv, kRingOcc);
                    if (occ == (1u << kPoolRing) - 1) break;
                    free_slot = __builtin_ctz(~occ);
                }
                unsigned b = 0;
                if (lane == 0) b = atomicAdd(work, 1u);
                b = __builtin_amdgcn_readfirstlane(b);
                if (b >= n_blocks) {
                    exhausted = true;
                    break;
                }
                // group-major (b = grp * n_tiles + tile) or, under a tile order, tile-major
                // (b = tile * n_groups + grp; KParams.deal_div). Two forms of the same mapping: the
                // branch kept the spheres variant's code as it was (a select moved it, C2 +1.1 %),
                // the select the final variant's (the branch added 8 B of spill to its ring kernel)
                unsigned grp, tile;
                if constexpr (C::F == FEAT_SET_SPHERES) {
                    if (__builtin_expect(P.tile_major != 0, 0)) {   // (wave-uniform)
                        tile = b / P.deal_div;
                        grp = b - tile * P.deal_div;
                        if constexpr (DealCfg<C>()) {
                            // A whole frame's deal order: position -> raster tile through the table
                            // behind the work counter (kDealTable), one scalar load per block off a
                            // pointer the wave holds anyway. Everything here reads registers the
                            // loop keeps live already (work, n_tiles, tile_major, tx0 / tk0): one
                            // more scalar value live through the walk costs the kernel a spill in
                            // its bounce loop (C2 +9.5 %).
                            if (P.tile_major >= kDealOrdered) {
                                tile = work[kDealTable + tile];
                                if (ring) b = tile * P.deal_div + grp;   // the ring keeps the raster tile's block id
                                // Block-cost measurement: a wave's cycles between two fetches go to
                                // the tile of the block fetched first. No state of its own: the
                                // previous tile is the one tx0 / tk0 still name (blk_units 0: none
                                // yet); lane 0 adds the fetch time to that tile's cost and subtracts
                                // it from the new tile's, so a tile's sum (mod 2^32) is its blocks'
                                // (next fetch - own fetch); the wave's last block is closed at its end.
                                if (P.tile_major == kDealMeasure) {
                                    const unsigned prev = (unsigned)(tk0 >> 3) * (unsigned)P.tiles_x + (unsigned)(tx0 >> 3);
                                    if ((blk_units == 0 || prev != tile) && lane == 0) {
                                        const unsigned now = (unsigned)__builtin_amdgcn_s_memtime();
                                        if (blk_units != 0) atomicAdd(&work[kDealTable + n_tiles + prev], now);
                                        atomicAdd(&work[kDealTable + n_tiles + tile], 0u - now);
                                    }
                                }
                            }
                        }
                    } else {
                        grp = b / n_tiles;
                        tile = b - grp * n_tiles;
                    }
                } else {
                    const unsigned outer = b / P.deal_div, inner = b - outer * P.deal_div;
                    grp = P.tile_major ? inner : outer;
                    tile = P.tile_major ? outer : inner;
                }
                tx0 = (int)(tile % (unsigned)P.tiles_x) * 8;
                tk0 = (int)(tile / (unsigned)P.tiles_x) * 8;
                vw = min(8, P.width - tx0);
                nvalid = (unsigned)(vw * min(8, P.n_rows - tk0));
                if constexpr (ITEMS) {
                    const unsigned chunk = grp * group;
                    s0 = P.sample_begin + (int)chunk * P.spp_chunk;
                    blk_units = nvalid * min(group, (unsigned)P.n_chunks - chunk);
                } else {
                    s0 = P.sample_begin + (int)(grp * group);
                    blk_units = nvalid * (unsigned)(min(P.spp, s0 + (int)group) - s0);
                    if (ring) {
                        if constexpr (RingSgpr<C>()) {   // the block id waits in the ring's header
                            if (lane == 0) ring_block_id(ring_of_wave<C>(P))[free_slot] = b;
                            cur_slot = (unsigned)free_slot;
                            occ |= 1u << free_slot;
                        }
                        if constexpr (!RingSgpr<C>()) {
                            ringv = ring_set((int)b, free_slot, ringv);
                            ringv = ring_set(free_slot, kRingCur, ringv);
                            ringv = ring_set((int)(occ | 1u << free_slot), kRingOcc, ringv);
                        }
                    }
                }
                blk_next = 0;
            }
            const unsigned rank = lanes_below(need);
            if constexpr (StagedPool<C, ITEMS>()) {
                // the block's sample row units are taken from, and the next pixel of it (wave-uniform)
                unsigned row, col;
                if (nvalid == 64u) {
                    row = blk_next >> 6;
                    col = blk_next & 63u;
                } else {
                    row = blk_next / nvalid;
                    col = blk_next - row * nvalid;
                }
                if (col == 0) {   // a new row: every pixel's sample start at once, one issue of the sequence per 64 samples
                    uint64_t t_stage = 0;
                    if (C::COUNT) t_stage = __builtin_amdgcn_s_memtime();
                    if ((unsigned)lane < nvalid) {
                        int px, pk;
                        if (nvalid == 64u) {
                            px = tx0 + (lane & 7);
                            pk = tk0 + (lane >> 3);
                        } else {
                            px = tx0 + (int)((unsigned)lane % (unsigned)vw);
                            pk = tk0 + (int)((unsigned)lane / (unsigned)vw);
                        }
                        int ix, y;
                        image_xy(P, px, pk, ix, y);
                        SeedSlot sl;
                        ds_start(sl.st, P.seed, (uint32_t)y * (uint32_t)P.img_width + (uint32_t)ix, (uint32_t)(s0 + (int)row));
                        camera_begin(P, ix, y, sl.st, sl.u, sl.v);
                        seed_slots<C>(S)[threadIdx.x] = sl;
                    }
                    // Other lanes of this wave read the slots below, and in later passes: a wave's LDS
                    // accesses complete in program order, so keeping the compiler from moving them
                    // across this point orders them; no workgroup barrier (the area is the wave's own).
                    // The previous row was taken to its last unit before this one was written.
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                    if (C::COUNT && lane == 0) {   // staging ran inside the refill: its time is seeding + jitter
                        const uint64_t dt = __builtin_amdgcn_s_memtime() - t_stage;   // (the counters are summed over lanes,
                        cnt.t_seed += dt;                                           // mod 2^64: one lane moves the interval)
                        cnt.t_refill -= dt;
                        cnt.cam_steps++;
                    }
                }
                // a pass never crosses a row (the loop's next pass stages and takes from the next one)
                const unsigned take = min(min((unsigned)__popcll(need), nvalid - col), blk_units - blk_next);
                if (!active && rank < take) {
                    const unsigned p = col + rank;
                    if (nvalid == 64u) {
                        x = tx0 + (int)(p & 7u);
                        k = tk0 + (int)(p >> 3);
                    } else {
                        x = tx0 + (int)(p % (unsigned)vw);
                        k = tk0 + (int)(p / (unsigned)vw);
                    }
                    s = s0 + (int)row;
                    if (ring) s |= (int)((cur_slot * kRingSlot + row * 64u + (unsigned)((k & 7) * 8 + (x & 7))) << kRingSampleBits);
                    const SeedSlot sl = seed_slots<C>(S)[(threadIdx.x & ~63u) + p];
                    st = sl.st;
                    r.dx = sl.u;
                    r.dy = sl.v;
                    Tr = Tg = Tb = (R)1;
                    cr = cg = cb = 0.0;
                    depth = P.max_depth;
                    if (C::COUNT) {
                        cnt.cam_lanes++;
                        t_sample = __builtin_amdgcn_s_memtime();
                    }
                    active = true;
                    new_sample = true;
                }
                blk_next += take;
                need = __ballot(!active);
                continue;
            }
            const unsigned take = min((unsigned)__popcll(need), blk_units - blk_next);
            if (!active && rank < take) {
                const unsigned u = blk_next + rank;
                unsigned si;
                if (nvalid == 64u) {  // a full 8x8 tile (wave-uniform): shifts, not divisions
                    si = u >> 6;
                    x = tx0 + (int)(u & 7u);
                    k = tk0 + (int)((u >> 3) & 7u);
                } else {
                    si = u / nvalid;
                    const unsigned p = u - si * nvalid;
                    x = tx0 + (int)(p % (unsigned)vw);
                    k = tk0 + (int)(p / (unsigned)vw);
                }
                if constexpr (ITEMS) {  // si: the item's chunk within the block; s its first sample
                    s = s0 + (int)si * P.spp_chunk;
                    left = min(P.spp, s + P.spp_chunk) - s - 1;
                    cr = cg = cb = 0.0;
                } else {
                    s = s0 + (int)si;
                    if (ring) {
                        if constexpr (!RingSgpr<C>()) cur_slot = (unsigned)__builtin_amdgcn_readlane(ringv, kRingCur);
                        s |= (int)((cur_slot * kRingSlot + si * 64u + (unsigned)((k & 7) * 8 + (x & 7))) << kRingSampleBits);
                    }
                }
                active = true;
                new_sample = true;
            }
            blk_next += take;
            need = __ballot(!active);
        }
        if (!__any(active)) break;
        if (C::COUNT && first_active_lane()) cnt.wave_steps++;
        if (C::COUNT) {   // lanes the refill left idle: nothing left to take, or (RING) no free slot
            const uint64_t idle = __ballot(!active);
            if (first_active_lane()) {
                if (exhausted) cnt.idle_tail += (uint32_t)__popcll(idle);
                else cnt.idle_ring += (uint32_t)__popcll(idle);
            }
        }
        if (!active) continue;
        // (COUNT) refill and loop overhead since the last iteration's end stamp: lanes refilled this
        // iteration were idle, so their stamp is old — take the wave's latest (max over lanes)
        if (C::COUNT) {
            unsigned long long tw = t_prev;
            for (int off = 32; off > 0; off >>= 1) {
                const unsigned long long o = __shfl_xor(tw, off);
                tw = tw > o ? tw : o;
            }
            t_prev = tw;
            RT_STAMP(cnt.t_refill, t_prev);
        }
        // Ray generation: the camera rays of new samples and the scattered rays of last
        // iteration's hits (pending), whose random_in_unit_disk / random_in_unit_sphere tries
        // run in one rejection loop (the wave used to run the two loops one after the other).
        // Each lane's draws keep their order (its stream is its own), so the bits do not change.
        bool go = true;   // the lane traces this iteration
        bool gen_wait = false;   // RT_TRY_LEFT: the lane's tries go on in the next iteration
        if constexpr (PrimaryPool<C, ITEMS>())
            generate_primary<C>(S, P, x, k, depth, new_sample, pending, st, r, h, Tr, Tg, Tb, cr, cg, cb, go, gen_wait, cnt);
        if constexpr (!PrimaryPool<C, ITEMS>()) {
            R u = 0, v = 0;
            bool tries = false;
            if (new_sample) {
                if constexpr (StagedPool<C, ITEMS>()) {
                    // the refill left the lane as camera_begin leaves it: every new sample's jitter waits
                    // in r.dx / r.dy (cam_wait is implied; the spheres variant reads no key.pixel / key.sample)
                    u = r.dx;
                    v = r.dy;
                } else if (TryLeft<C>() && cam_wait) {   // camera_begin ran: the jitter waits in r.dx / r.dy
                    u = r.dx;
                    v = r.dy;
                    cam_wait = false;
                } else {
                    if (C::COUNT) {
                        cnt.cam_lanes++;
                        if (first_active_lane()) cnt.cam_steps++;
                    }
                    int ix, y;
                    image_xy(P, x, k, ix, y);
                    if (C::COUNT) t_sample = __builtin_amdgcn_s_memtime();
                    key.pixel = (uint32_t)y * (uint32_t)P.img_width + (uint32_t)ix;
                    const uint32_t sample = ring ? (uint32_t)s & kRingSampleMask : (uint32_t)s;
                    key.sample = sample;
                    if constexpr (C::F32) ds_start_f32(st, P.seed, key.pixel, sample);
                    else ds_start(st, P.seed, key.pixel, sample);
                    camera_begin(P, ix, y, st, u, v);
                    Tr = Tg = Tb = (R)1;
                    if constexpr (!ITEMS) cr = cg = cb = 0.0;  // ITEMS: the chunk's running sum
                    depth = P.max_depth;
                }
                tries = true;
            } else if (pending) {
                tries = shade_draws<C>(S, h.mat);
            }
            RT_STAMP(cnt.t_seed, t_prev);
            R qx = (R)0, qy = (R)0, qz = (R)0, l2 = (R)1;
            const bool three = !new_sample;
            if constexpr (TryLeft<C>()) {
                bool accepted = !tries;
                for (int n = 1;; ++n) {
                    if (!accepted) accepted = unit_try(st, (R)P.scale_m11, three, qx, qy, qz, l2);
                    const uint64_t rejecting = __ballot(!accepted);
                    if (rejecting == 0 || (n >= RT_TRY_MIN && __popcll(rejecting) <= RT_TRY_LEFT)) break;
                }
                gen_wait = !accepted;
            } else {
                while (tries && !unit_try(st, (R)P.scale_m11, three, qx, qy, qz, l2)) {
                }
            }
            RT_STAMP(cnt.t_tries, t_prev);
            if (gen_wait) {   // (RT_TRY_LEFT) no trace this iteration; pending / new_sample stay set
                go = false;
                if (new_sample) {
                    cam_wait = true;
                    r.dx = u;
                    r.dy = v;
                }
            } else if (new_sample) {
                new_sample = false;
                camera_end(P, st, u, v, qx, qy, r);
            } else if (pending) {
                pending = false;
                go = shade_end<C, false>(S, h, r, st, Tr, Tg, Tb, qx, qy, qz, l2);
                if (go) depth -= 1;
            }
        }
        RT_STAMP(t_cam, t_prev);
        if (C::COUNT) {
            cnt.try_wait += gen_wait ? 1u : 0u;
            cnt.no_scatter += (!go && !gen_wait) ? 1u : 0u;
            cnt.depth_cap += (go && depth <= 0) ? 1u : 0u;
        }
        if (go && depth > 0) {  // main.rs:21-23: depth 0 is black
            key.bounce = (uint32_t)(P.max_depth - depth);
            if (C::COUNT) cnt.casts++;
            finish_ray<C>(r, S.has_spheres != 0);
            forget(h);
            RT_STAMP(cnt.t_setup, t_prev);
            const bool hit = trace_world<C>(S, r, h, stack, key, cnt);
            if (C::COUNT) t_prev = __builtin_amdgcn_s_memtime();   // trace_world stamped its phases
            if (!hit) {  // main.rs:37: background
                cr = cr + Tr * P.bg[0];
                cg = cg + Tg * P.bg[1];
                cb = cb + Tb * P.bg[2];
            } else {
                if (C::COUNT) {
                    cnt.shade_lanes++;
                    if (first_active_lane()) cnt.shade_steps++;
                }
                pending = shade_begin<C>(S, h, Tr, Tg, Tb, cr, cg, cb);
            }
            RT_STAMP(t_shade, t_prev);
        }
        if (C::COUNT) t_prev = __builtin_amdgcn_s_memtime();   // lanes that did not trace
        if (C::COUNT && P.tile_cost && !(pending || gen_wait)) {   // the sample ended: its lane-cycles to its tile
            int ix, y;
            image_xy(P, x, k, ix, y);
            atomicAdd(&P.tile_cost[(unsigned)(y >> 3) * (unsigned)P.img_tiles_x + (unsigned)(ix >> 3)],
                      (unsigned long long)(t_prev - t_sample));
        }
        if (pending || gen_wait) {
        } else if (ITEMS && left > 0) {  // the item's next sample: the lane takes it at the loop top
            active = false;
            own = true;
        } else {
            // items: the chunk's partial, [chunk][pixel]; per-sample pool: tiled_record order,
            // or (ring) the record index taken with the unit (in the high bits of s)
            double* o;
            if (ITEMS) {
                o = samples + ((size_t)((unsigned)(s - P.sample_begin) / (unsigned)P.spp_chunk) * n_px +
                               (size_t)k * P.width + x) * 3;
            } else if (ring) {
                o = ring_of_wave<C>(P) + (size_t)((unsigned)s >> kRingSampleBits) * 3;
            } else {
                o = samples + tiled_record(P.tiles_x, P.spp - P.sample_begin, x, k, s - P.sample_begin) * 3;
            }
            if constexpr (C::F32 && !ITEMS && !ring) {
                // the f32 mode's per-sample records are f32 (SampleTiles.f32_records): half the bytes
                float* of = reinterpret_cast<float*>(samples) +
                            tiled_record(P.tiles_x, P.spp - P.sample_begin, x, k, s - P.sample_begin) * 3;
                of[0] = (float)cr;
                of[1] = (float)cg;
                of[2] = (float)cb;
                (void)o;
            } else {
                o[0] = cr;
                o[1] = cg;
                o[2] = cb;
            }
            active = false;
        }
    }
    if constexpr (DealCfg<C>()) {   // the wave's last block ends with the wave
        if (P.tile_major == kDealMeasure && blk_units != 0 && lane == 0)
            atomicAdd(&work[kDealTable + n_tiles + (unsigned)(tk0 >> 3) * (unsigned)P.tiles_x + (unsigned)(tx0 >> 3)],
                      (unsigned)__builtin_amdgcn_s_memtime());
    }
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
        // phase times: each region's first active lane added its intervals, so every lane's
        // share goes in (trace = everything from the ray set-up to the hit record)
        const uint64_t trace = cnt.t_setup + cnt.t_pre + cnt.t_nodes + cnt.t_leaves + cnt.t_defer + cnt.t_rec;
        atomicAdd(&counters[kCtrCyclesCamera], (unsigned long long)(t_cam + cnt.t_seed + cnt.t_tries));   // ray generation, all of it
        atomicAdd(&counters[kCtrCyclesSeed], (unsigned long long)cnt.t_seed);
        atomicAdd(&counters[kCtrCyclesTries], (unsigned long long)cnt.t_tries);
        atomicAdd(&counters[kCtrCyclesTrace], (unsigned long long)trace);
        atomicAdd(&counters[kCtrCyclesShade], (unsigned long long)t_shade);
        atomicAdd(&counters[kCtrCyclesNodes], (unsigned long long)cnt.t_nodes);
        atomicAdd(&counters[kCtrCyclesLeaves], (unsigned long long)cnt.t_leaves);
        atomicAdd(&counters[kCtrCyclesSetup], (unsigned long long)cnt.t_setup);
        atomicAdd(&counters[kCtrCyclesPre], (unsigned long long)cnt.t_pre);
        atomicAdd(&counters[kCtrCyclesRecord], (unsigned long long)cnt.t_rec);
        atomicAdd(&counters[kCtrCyclesMedia], (unsigned long long)cnt.t_med);
        atomicAdd(&counters[kCtrCyclesInstances], (unsigned long long)cnt.t_inst);
        atomicAdd(&counters[kCtrCyclesRefill], (unsigned long long)cnt.t_refill);
        atomicAdd(&counters[kCtrCyclesDeferred], (unsigned long long)cnt.t_defer);
        atomicAdd(&counters[kCtrIdleTail], (unsigned long long)cnt.idle_tail);
        atomicAdd(&counters[kCtrIdleRing], (unsigned long long)cnt.idle_ring);
        atomicAdd(&counters[kCtrNoScatter], (unsigned long long)cnt.no_scatter);
        atomicAdd(&counters[kCtrDepthCap], (unsigned long long)cnt.depth_cap);
        atomicAdd(&counters[kCtrTryWait], (unsigned long long)cnt.try_wait);
        if (lane == 0) {   // the wave's lifetime; the longest, and the wave count (the launch's tail)
            const unsigned long long life = __builtin_amdgcn_s_memtime() - t_start;
            atomicAdd(&counters[kCtrCyclesKernel], life);
            atomicMax(&counters[kCtrLongestWave], life);
            atomicAdd(&counters[kCtrWaves], 1ull);
        }
    }
}

}  // namespace rtk
