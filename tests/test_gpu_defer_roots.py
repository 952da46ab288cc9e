"""RT_OPT_DEFER_ROOTS on the GPU (csrc/root_bracket.hpp, trace_walk.hpp trace_world_defer, trace_pool's
CfgDefer instantiations): where the primary-candidate kernel runs, its sphere tests decide from f32
brackets of the roots and only a cast's winner gets its exact f64 root.

The brackets only ever replace a decision the exact roots would have taken the same way, and the
winner's root is sphere_t's, so no bit may change: every comparison here is the frame (and the
sample count) with the option on against the option off, np.array_equal, at max_depth 50 and 1.
Scene 0 under a long lens (at most 10 % of the pixels flagged "walk", so the candidate loop runs
nearly everywhere) at 64x48x8 and 156x92x4 (edge tiles of 4 columns and 4 rows): the per-sample
buffer, the forced ring, a 2-way tile shard, an adaptive pass, RT_OPT_HOIST 0 (the r = 1000 sphere
inside the walk, through the brackets); RT_OPT_PRIMARY_CANDIDATES 0, where the option is inert and
rt_stats says so; the generated worlds; coincident and 1e-12-apart spheres. All inputs are finite:
the NaN cases are the CPU's (tests/test_root_bracket.py).
"""
import numpy as np
import pytest

from tests import generated_worlds as gw

pytestmark = pytest.mark.gpu

SIZES = [(64, 48, 8), (156, 92, 4)]
DEPTHS = [50, 1]


def _long_lens(rt, W, H):
    # test_gpu_primary_candidates.py's second camera: a 12-degree field of view, a small aperture
    return rt.camera_new((-4.0, 3.0, 9.0), (1.0, 0.5, 0.0), (0.0, 1.0, 0.0), 12.0, W / H, 0.05, 9.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    world = rt.World(1).build_scene(0)
    r.upload(world)
    r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
    yield r, world
    r.close()


def _render(rt, r, cam, bg, W, H, spp, depth, defer, ring=0, primary=1, **kw):
    r.set_schedule(rt.RT_SCHED_POOL)
    r.set_option(rt.RT_OPT_POOL_RING, ring)
    r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES, primary)
    r.set_option(rt.RT_OPT_DEFER_ROOTS, 1 if defer else 0)
    try:
        img = r.render(cam, rt.Renderer.params(W, H, spp, depth, bg, 1, out_format=rt.RT_OUT_F64, **kw))
        st = r.stats()
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
        r.set_option(rt.RT_OPT_POOL_RING, 1)
        r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES, 1)
        r.set_option(rt.RT_OPT_DEFER_ROOTS, 1)
    assert st.schedule == rt.RT_SCHED_POOL and (st.ring_bytes > 0) == (ring == 2)
    # which kernel ran: the deferred one exactly where the option is on and a candidate table was used
    assert st.defer_roots == (1 if defer and st.primary_table_bytes > 0 else 0)
    return img, st


def _same(on, off, what):
    (a, sa), (b, sb) = on, off
    assert np.isfinite(b).all()
    assert np.array_equal(a, b), "%s: %d px differ, max |d| %.3e" % (
        what, int((a != b).any(axis=-1).sum()), float(np.abs(a - b).max()))
    assert sa.samples == sb.samples and sa.n_batches == sb.n_batches


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("ring", [0, 2], ids=["buffer", "ring"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_on_equals_off(rt, ctx, size, ring, depth):
    r, _ = ctx
    W, H, spp = size
    cam, bg = _long_lens(rt, W, H), (0.7, 0.8, 1.0)
    off = _render(rt, r, cam, bg, W, H, spp, depth, False, ring)
    on = _render(rt, r, cam, bg, W, H, spp, depth, True, ring)
    _same(on, off, "%dx%dx%d depth %d ring %d" % (W, H, spp, depth, ring))
    assert on[1].defer_roots == 1 and off[1].defer_roots == 0 and off[1].primary_table_bytes == 16 * W * H
    assert on[1].primary_walk_share <= 0.10     # the candidate loop, not the walk, resolves nearly every primary ray
    if depth > 1:
        assert off[0].max() > 0
    else:
        # at depth 1 a hit is black and the long lens sees no sky: the scene's own camera too, which does
        cam, bg = rt.scene_camera(0, W, H)
        off = _render(rt, r, cam, bg, W, H, spp, depth, False, ring)
        on = _render(rt, r, cam, bg, W, H, spp, depth, True, ring)
        _same(on, off, "scene camera, %dx%dx%d depth %d ring %d" % (W, H, spp, depth, ring))
        assert on[1].defer_roots == 1 and off[0].max() > 0


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_two_way_tile_shard(rt, ctx, size, depth):
    r, _ = ctx
    W, H, spp = size
    cam, bg = _long_lens(rt, W, H), (0.7, 0.8, 1.0)
    for begin in (0, 1):
        kw = dict(row_begin=begin, row_stride=2, tile_shard=1)
        off = _render(rt, r, cam, bg, W, H, spp, depth, False, **kw)
        on = _render(rt, r, cam, bg, W, H, spp, depth, True, **kw)
        _same(on, off, "tile shard %d of 2, depth %d" % (begin, depth))
        assert on[1].defer_roots == 1


@pytest.mark.parametrize("depth", DEPTHS)
def test_one_adaptive_pass(rt, ctx, depth):
    """The first pass at 4 spp, then one adaptive pass to the cap of 8: tile shards under the call's order."""
    r, _ = ctx
    W, H = 156, 92
    cam, bg = _long_lens(rt, W, H), (0.7, 0.8, 1.0)
    p = rt.Renderer.params(W, H, 8, depth, bg, 1, out_format=rt.RT_OUT_F64)
    out = {}
    for on in (0, 1):
        r.set_option(rt.RT_OPT_DEFER_ROOTS, on)
        try:
            out[on] = r.render_adaptive(cam, p, 4, 4, 0.0)
        finally:
            r.set_option(rt.RT_OPT_DEFER_ROOTS, 1)
    for a, b in zip(out[1], out[0]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("depth", DEPTHS)
def test_ground_sphere_inside_the_walk(rt, depth):
    """RT_OPT_HOIST 0: no pre-leaf, so the r = 1000 sphere is a leaf of the walk and goes through the
    brackets, whose error there is of the order of t_min for a ray that starts on it."""
    r = rt.Renderer(0)
    try:
        r.set_option(rt.RT_OPT_HOIST, 0)
        r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
        r.upload(rt.World(1).build_scene(0))
        W, H, spp = SIZES[0]
        cam, bg = _long_lens(rt, W, H), (0.7, 0.8, 1.0)
        for ring in (0, 2):
            off = _render(rt, r, cam, bg, W, H, spp, depth, False, ring)
            on = _render(rt, r, cam, bg, W, H, spp, depth, True, ring)
            _same(on, off, "hoist off, ring %d, depth %d" % (ring, depth))
            assert on[1].defer_roots == 1
    finally:
        r.close()


def test_inert_without_primary_candidates(rt, ctx):
    r, _ = ctx
    W, H, spp = SIZES[0]
    cam, bg = _long_lens(rt, W, H), (0.7, 0.8, 1.0)
    ref = _render(rt, r, cam, bg, W, H, spp, 50, False)
    for ring in (0, 2):
        off = _render(rt, r, cam, bg, W, H, spp, 50, False, ring, primary=0)
        on = _render(rt, r, cam, bg, W, H, spp, 50, True, ring, primary=0)
        _same(on, off, "no candidate table, ring %d" % ring)
        assert (on[1].defer_roots, off[1].defer_roots, on[1].primary_table_bytes) == (0, 0, 0)
        assert np.array_equal(on[0], ref[0])
    # the item pool, the chunk schedule and a count_work render keep their kernels too
    try:
        for sched, kw in ((rt.RT_SCHED_ITEMS, {}), (rt.RT_SCHED_CHUNKS, {}), (rt.RT_SCHED_POOL, dict(count_work=1))):
            r.set_schedule(sched)
            img = r.render(cam, rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=rt.RT_OUT_F64, **kw))
            assert r.stats().defer_roots == 0 and np.array_equal(img, ref[0])
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)


def test_generated_worlds(rt):
    """Every generated world renders the same with the option on and off; those the primary-candidate
    kernel runs (the spheres-only ones) run the deferred kernel, the others report that they did not."""
    ran = []
    for case in gw.SUPPORTED:
        r = rt.Renderer(0)
        try:
            r.upload(gw.build(rt, case).tw.product)
            r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
            cam = gw.camera(rt, case, gw.W, gw.H)
            for depth in DEPTHS:
                off = _render(rt, r, cam, case.bg, gw.W, gw.H, gw.SPP, depth, False)
                on = _render(rt, r, cam, case.bg, gw.W, gw.H, gw.SPP, depth, True)
                _same(on, off, "%s depth %d" % (case.name, depth))
            if on[1].defer_roots:
                assert on[1].variant_features == 0
                ran.append(case.name)
        finally:
            r.close()
    print("deferred kernel ran on:", ran)
    assert "inside_glass" in ran


def _pairs_world(rt, gap):
    """Pairs of spheres whose centres are `gap` apart along z (0: coincident, the later-tested one
    wins every tie), in different materials so that the winner shows, among filler spheres on a ground."""
    w = rt.World(1)
    mats = [w.lambertian(w.solid(0.8, 0.2, 0.2)), w.lambertian(w.solid(0.2, 0.8, 0.2)), w.metal((0.8, 0.8, 0.9), 0.0),
            w.dielectric(1.5)]
    for i in range(24):
        w.push(w.sphere(mats[i % 4], (-5.5 + 1.0 * (i % 12), 0.35, -3.0 + 1.1 * (i // 12)), 0.3))
    for i in range(6):
        c = (-3.0 + 1.2 * i, 0.5, 1.0)
        w.push(w.sphere(mats[i % 4], c, 0.5))
        w.push(w.sphere(mats[(i + 1) % 4], (c[0], c[1], c[2] + gap), 0.5))
    w.push(w.sphere(w.lambertian(w.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), (0.0, -1000.0, 0.0), 1000.0))
    return w


@pytest.mark.parametrize("gap", [0.0, 1e-12], ids=["coincident", "1e-12 apart"])
def test_coincident_spheres(rt, gap):
    r = rt.Renderer(0)
    try:
        r.upload(_pairs_world(rt, gap))
        r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
        W, H, spp = 64, 48, 8
        cam = rt.camera_new((0.0, 2.0, 9.0), (0.0, 0.5, 1.0), (0.0, 1.0, 0.0), 30.0, W / H, 0.05, 8.0, 0.0, 1.0)
        for depth in DEPTHS:
            for ring in (0, 2):
                off = _render(rt, r, cam, (0.7, 0.8, 1.0), W, H, spp, depth, False, ring)
                on = _render(rt, r, cam, (0.7, 0.8, 1.0), W, H, spp, depth, True, ring)
                _same(on, off, "gap %g depth %d ring %d" % (gap, depth, ring))
                assert on[1].defer_roots == 1 and on[1].variant_features == 0
                if depth > 1:
                    assert off[0].max() > 0
    finally:
        r.close()


def test_the_option_is_additive_and_checked(rt, ctx):
    r, _ = ctx
    assert r.get_option(rt.RT_OPT_DEFER_ROOTS) == 1
    for bad in (2, -1):
        with pytest.raises(rt.RTError):
            r.set_option(rt.RT_OPT_DEFER_ROOTS, bad)
    r.set_option(rt.RT_OPT_DEFER_ROOTS, 0)
    assert r.get_option(rt.RT_OPT_DEFER_ROOTS) == 0
    r.set_option(rt.RT_OPT_DEFER_ROOTS, 1)
