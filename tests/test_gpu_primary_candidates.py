"""RT_OPT_PRIMARY_CANDIDATES on the GPU (csrc/primary_candidates.hip, trace_pool's CfgPrimary
instantiations): a new sample of the f64 spheres variant's per-sample pool takes its first hit from
an exact test of its pixel's candidate list and joins the walk with its first bounce ray.

The candidate list is a superset of what a primary ray of the pixel can hit, the tests are the
walk's own and every lane's draws keep their order, so no bit may change: every comparison here is
the frame with the option on against the frame with it off, exact. Scene 0 (the random spheres) at
48x32x6, 37x21x17 and 9x5x1, max_depth 0, 1 and 50, the per-sample buffer and the in-kernel ring;
a tile shard; K forced to 1 (nearly every pixel falls back to the walk); a camera change between
two renders (the table is rebuilt); a new upload (the table is dropped); a world whose camera sits
inside a glass sphere.
"""
import numpy as np
import pytest

from tests import generated_worlds as gw

pytestmark = pytest.mark.gpu

SIZES = [(48, 32, 6), (37, 21, 17), (9, 5, 1)]
DEPTHS = [0, 1, 50]


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    world = rt.World(1).build_scene(0)
    r.upload(world)
    r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
    yield r, world
    r.close()


def _render(rt, r, cam, bg, W, H, spp, depth, on, ring=0, k=7, **kw):
    r.set_schedule(rt.RT_SCHED_POOL)
    r.set_option(rt.RT_OPT_POOL_RING, ring)
    r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES, 1 if on else 0)
    r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES_K, k)
    try:
        img = r.render(cam, rt.Renderer.params(W, H, spp, depth, bg, 1, out_format=rt.RT_OUT_F64, **kw))
        st = r.stats()
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
        r.set_option(rt.RT_OPT_POOL_RING, 1)
        r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES, 1)
        r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES_K, 7)
    assert st.schedule == rt.RT_SCHED_POOL and st.variant_features == 0 and (st.ring_bytes > 0) == (ring == 2)
    if on:
        assert st.primary_table_bytes == 16 * W * H and 0.0 <= st.primary_walk_share <= 1.0
    else:
        assert st.primary_table_bytes == 0 and st.primary_build_ms == 0.0 and st.primary_walk_share == 0.0
    return img, st


def _same(got, ref, what):
    assert np.isfinite(ref).all()
    assert np.array_equal(got, ref), "%s: %d px differ, max |d| %.3e" % (
        what, int((got != ref).any(axis=-1).sum()), float(np.abs(got - ref).max()))


@pytest.mark.parametrize("ring", [0, 2], ids=["buffer", "ring"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_on_equals_off(rt, ctx, size, ring):
    r, _ = ctx
    W, H, spp = size
    cam, bg = rt.scene_camera(0, W, H)
    for depth in DEPTHS:
        off, _ = _render(rt, r, cam, bg, W, H, spp, depth, False, ring)
        on, st = _render(rt, r, cam, bg, W, H, spp, depth, True, ring)
        _same(on, off, "%dx%dx%d depth %d ring %d" % (W, H, spp, depth, ring))
        assert st.primary_walk_share < 1.0      # some pixels are listed: the new path ran
        if depth > 0:
            assert off.max() > 0


@pytest.mark.parametrize("size", SIZES[:2], ids=lambda s: "%dx%dx%d" % s)
def test_tile_shard(rt, ctx, size):
    """A tile shard's grid is whole 8x8 tiles: at 37x21 its edge tiles hold pixels beyond the frame,
    which have no record and walk."""
    r, _ = ctx
    W, H, spp = size
    cam, bg = rt.scene_camera(0, W, H)
    kw = dict(row_begin=1, row_stride=3, tile_shard=1)
    for ring in (0, 2):
        off, _ = _render(rt, r, cam, bg, W, H, spp, 50, False, ring, **kw)
        on, _ = _render(rt, r, cam, bg, W, H, spp, 50, True, ring, **kw)
        _same(on, off, "tile shard, ring %d" % ring)
        assert off.max() > 0


def test_adaptive_passes(rt, ctx):
    """rt_render_adaptive's passes are tile shards under the call's own order, edge tiles whole."""
    r, _ = ctx
    W, H, spp = 37, 21, 17
    cam, bg = rt.scene_camera(0, W, H)
    p = rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=rt.RT_OUT_F64)
    out = {}
    for on in (0, 1):
        r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES, on)
        try:
            out[on] = r.render_adaptive(cam, p, 8, 4, 0.0)
        finally:
            r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES, 1)
    for a, b in zip(out[1], out[0]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_k_forced_to_one(rt, ctx, size):
    r, _ = ctx
    W, H, spp = size
    cam, bg = rt.scene_camera(0, W, H)
    off, _ = _render(rt, r, cam, bg, W, H, spp, 50, False)
    on7, st7 = _render(rt, r, cam, bg, W, H, spp, 50, True, k=7)
    on1, st1 = _render(rt, r, cam, bg, W, H, spp, 50, True, k=1)
    _same(on1, off, "k = 1")
    _same(on7, off, "k = 7")
    assert st1.primary_build_ms > 0.0 and st1.primary_walk_share >= st7.primary_walk_share
    if W > 9:
        assert st1.primary_walk_share > st7.primary_walk_share


def test_camera_change_and_upload_rebuild_the_table(rt, ctx):
    r, world = ctx
    W, H, spp = 37, 21, 17
    cam_a, bg = rt.scene_camera(0, W, H)
    cam_b = rt.camera_new((-4.0, 3.0, 9.0), (1.0, 0.5, 0.0), (0.0, 1.0, 0.0), 12.0, W / H, 0.05, 9.0, 0.0, 1.0)
    off_a, _ = _render(rt, r, cam_a, bg, W, H, spp, 50, False)
    off_b, _ = _render(rt, r, cam_b, bg, W, H, spp, 50, False)
    assert not np.array_equal(off_a, off_b)
    r.upload(world)     # nothing cached
    on_a, st = _render(rt, r, cam_a, bg, W, H, spp, 50, True)
    assert st.primary_build_ms > 0.0
    on_a2, st = _render(rt, r, cam_a, bg, W, H, spp, 50, True)
    assert st.primary_build_ms == 0.0       # the same key: reused
    on_b, st_b = _render(rt, r, cam_b, bg, W, H, spp, 50, True)
    assert st_b.primary_build_ms > 0.0      # another camera: rebuilt
    on_a3, st = _render(rt, r, cam_a, bg, W, H, spp, 50, True)
    assert st.primary_build_ms > 0.0
    r.upload(world)
    on_a4, st = _render(rt, r, cam_a, bg, W, H, spp, 50, True)
    assert st.primary_build_ms > 0.0        # a new upload: dropped with the deal cache
    for got in (on_a, on_a2, on_a3, on_a4):
        _same(got, off_a, "camera a")
    _same(on_b, off_b, "camera b")


def test_camera_inside_a_glass_sphere(rt):
    case = next(c for c in gw.SUPPORTED if c.name == "inside_glass")
    r = rt.Renderer(0)
    try:
        r.upload(gw.build(rt, case).tw.product)
        r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
        for W, H, spp in SIZES:
            cam = gw.camera(rt, case, W, H)
            off, _ = _render(rt, r, cam, case.bg, W, H, spp, 50, False)
            on, st = _render(rt, r, cam, case.bg, W, H, spp, 50, True)
            _same(on, off, "inside_glass %dx%dx%d" % (W, H, spp))
            assert off.max() > 0
    finally:
        r.close()


def test_the_option_is_additive_and_checked(rt, ctx):
    r, _ = ctx
    assert r.get_option(rt.RT_OPT_PRIMARY_CANDIDATES) == 1 and r.get_option(rt.RT_OPT_PRIMARY_CANDIDATES_K) == 7
    for key, bad in ((rt.RT_OPT_PRIMARY_CANDIDATES, 2), (rt.RT_OPT_PRIMARY_CANDIDATES, -1),
                     (rt.RT_OPT_PRIMARY_CANDIDATES_K, 0), (rt.RT_OPT_PRIMARY_CANDIDATES_K, 8)):
        with pytest.raises(rt.RTError):
            r.set_option(key, bad)
    # the item pool, the chunk schedule and a count_work render keep their kernels: nothing is built
    W, H = 48, 32
    cam, bg = rt.scene_camera(0, W, H)
    try:
        for sched, kw in ((rt.RT_SCHED_ITEMS, {}), (rt.RT_SCHED_CHUNKS, {}), (rt.RT_SCHED_POOL, dict(count_work=1))):
            r.set_schedule(sched)
            r.render(cam, rt.Renderer.params(W, H, 4, 8, bg, 1, out_format=rt.RT_OUT_F64, **kw))
            assert r.stats().primary_table_bytes == 0
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
