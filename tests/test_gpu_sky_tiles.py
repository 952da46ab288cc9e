"""RT_OPT_SKIP_SKY_TILES on the GPU (csrc/primary_candidates.hip primary_sky_tiles, abi.cpp deal_setup,
trace_kernel.hip reduce_samples_tiled): an 8x8 tile whose pixels' candidate lists are all empty is
never dealt to the trace kernel, and the reduction sums 0.0 + 1.0 * background in its records' place.

Every sample of such a pixel is exactly that constant and the reduction's additions keep their order,
so no bit may change: every comparison here is the frame with the option on against the frame with
it off, exact. Scene 0 at 156x92x4 (35 of 240 tiles all sky; an edge column and an edge row of half
tiles) and 64x48x3 (3 of 48), three renders in a row per setting so that the measuring render, the
one that builds the cost order and an ordered one all run, under RT_OPT_AUTO_DEAL_ORDER 0, 1 and 2.
The skip needs a deal table: under mode 0 there is none and rt_stats.sky_tiles is 0 (DESIGN.md
§5.2); under 1 and 2 it is the host twin's count. Also: the option changed between two renders of one
key (the device tables are rewritten), a background other than the preset's, max_depth 0, a tile
shard, a progressive render and the in-kernel ring (none of them skips), a camera change and a
new upload (the flags are rebuilt with the table).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(156, 92, 4), (64, 48, 3)]
K = 7


@pytest.fixture(scope="module")
def ctx(rt):
    r = rt.Renderer(0)
    world = rt.World(1).build_scene(0)
    r.upload(world)
    soa = world.flatten(rt.RT_ACCEL_SAH)
    yield r, world, soa
    r.close()


def _render(rt, r, cam, bg, W, H, spp, depth, on, deal=1, ring=0, **kw):
    r.set_schedule(rt.RT_SCHED_POOL)
    r.set_option(rt.RT_OPT_POOL_RING, ring)
    r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, deal)
    r.set_option(rt.RT_OPT_SKIP_SKY_TILES, 1 if on else 0)
    try:
        img = r.render(cam, rt.Renderer.params(W, H, spp, depth, bg, 1, out_format=rt.RT_OUT_F64, **kw))
        st = r.stats()
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
        r.set_option(rt.RT_OPT_POOL_RING, 1)
        r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 1)
        r.set_option(rt.RT_OPT_SKIP_SKY_TILES, 1)
    assert st.schedule == rt.RT_SCHED_POOL and st.variant_features == 0 and (st.ring_bytes > 0) == (ring == 2)
    return img, st


def _same(got, ref, what):
    assert np.isfinite(ref).all()
    assert np.array_equal(got, ref), "%s: %d px differ, max |d| %.3e" % (
        what, int((got != ref).any(axis=-1).sum()), float(np.abs(got - ref).max()))


def _sky_pixels(flags, W, H):
    """The frame's pixels inside flagged tiles, (H, W) bool."""
    return np.kron(flags, np.ones((8, 8), np.uint8))[:H, :W].astype(bool)


@pytest.mark.parametrize("deal", [0, 1, 2])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_on_equals_off_over_three_renders(rt, ctx, size, deal):
    r, world, soa = ctx
    W, H, spp = size
    cam, bg = rt.scene_camera(0, W, H)
    flags, n_sky = rt.primary_sky_tiles_host(soa, cam, W, H, K)
    assert 0 < n_sky < flags.size
    frames = {}
    for on in (False, True):
        r.upload(world)     # nothing cached: the first render measures, the second builds the order, the third is ordered
        for i in range(3):
            img, st = _render(rt, r, cam, bg, W, H, spp, 50, on, deal)
            assert st.primary_table_bytes == 16 * W * H and (st.primary_build_ms > 0.0) == (i == 0)
            assert st.sky_tiles == (n_sky if on and deal != 0 else 0), (on, deal, i, st.sky_tiles)
            assert len(r.deal_order()) == (flags.size if deal == 1 and i > 0 else 0)
            frames[on, i] = img
    for i in range(3):
        _same(frames[True, i], frames[False, i], "%dx%dx%d deal %d render %d" % (W, H, spp, deal, i))
        _same(frames[False, i], frames[False, 0], "off, render %d against render 0" % i)
    sky = _sky_pixels(flags, W, H)
    assert frames[False, 0][~sky].max() > 0
    # a skipped pixel is the mean of spp backgrounds
    want = np.zeros(3)
    for _ in range(spp):
        want = want + np.asarray(bg, np.float64)
    assert np.array_equal(frames[True, 0][sky], np.broadcast_to(want * (1.0 / spp), (int(sky.sum()), 3)))


def test_the_option_may_change_between_renders_of_one_key(rt, ctx):
    """The device's deal tables are rewritten when what they leave out is not what the render wants."""
    r, world, soa = ctx
    W, H, spp = SIZES[0]
    cam, bg = rt.scene_camera(0, W, H)
    _, n_sky = rt.primary_sky_tiles_host(soa, cam, W, H, K)
    ref, _ = _render(rt, r, cam, bg, W, H, spp, 50, False, 0)
    for first in (False, True):
        r.upload(world)
        on = first
        for i in range(6):      # measure, build, then ordered renders, the option flipped every time
            img, st = _render(rt, r, cam, bg, W, H, spp, 50, on, 1)
            assert st.sky_tiles == (n_sky if on else 0)
            _same(img, ref, "flip %d (on %d)" % (i, on))
            order = r.deal_order()
            if i > 0:
                assert sorted(order.tolist()) == list(range(240))      # the cache's own order stays whole
            on = not on


def test_another_background(rt, ctx):
    r, world, soa = ctx
    W, H, spp = SIZES[0]
    cam, _ = rt.scene_camera(0, W, H)
    bg = (0.1, 0.2, 0.3)
    flags, n_sky = rt.primary_sky_tiles_host(soa, cam, W, H, K)
    r.upload(world)
    for i in range(3):
        off, st0 = _render(rt, r, cam, bg, W, H, spp, 50, False)
        on, st1 = _render(rt, r, cam, bg, W, H, spp, 50, True)
        assert (st0.sky_tiles, st1.sky_tiles) == (0, n_sky)
        _same(on, off, "bg (0.1, 0.2, 0.3), render %d" % i)
    sky = _sky_pixels(flags, W, H)
    assert np.abs(on[sky] - np.asarray(bg)).max() < 1e-15 and np.abs(on[~sky] - np.asarray(bg)).max() > 1e-3


def test_renders_that_keep_every_tile(rt, ctx):
    """max_depth 0 (the frame is black, not the background), a tile shard, the in-kernel ring and a
    progressive render report sky_tiles == 0, and their frames do not depend on the option."""
    r, world, _ = ctx
    W, H, spp = SIZES[0]
    cam, bg = rt.scene_camera(0, W, H)
    cases = [("depth 0", 0, 0, {}), ("tile shard", 50, 0, dict(row_begin=1, row_stride=3, tile_shard=1)),
             ("ring", 50, 2, {})]
    for what, depth, ring, kw in cases:
        r.upload(world)
        for i in range(2):
            off, st0 = _render(rt, r, cam, bg, W, H, spp, depth, False, ring=ring, **kw)
            on, st1 = _render(rt, r, cam, bg, W, H, spp, depth, True, ring=ring, **kw)
            assert (st0.sky_tiles, st1.sky_tiles) == (0, 0), what
            _same(on, off, what)
        if depth == 0:
            assert not on.any()
    # after a skipping render of the key: the shard and the black frame still see every tile
    full, st = _render(rt, r, cam, bg, W, H, spp, 50, True)
    assert st.sky_tiles > 0
    black, st = _render(rt, r, cam, bg, W, H, spp, 0, True)
    assert st.sky_tiles == 0 and not black.any()
    p = rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=rt.RT_OUT_F64)
    r.set_schedule(rt.RT_SCHED_POOL)
    r.set_option(rt.RT_OPT_POOL_RING, 0)
    try:
        prog = r.render_progressive(cam, p, 2)
        assert r.stats().sky_tiles == 0
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
        r.set_option(rt.RT_OPT_POOL_RING, 1)
    _same(prog, full, "progressive")


def test_camera_change_and_upload_rebuild_the_flags(rt, ctx):
    r, world, soa = ctx
    W, H, spp = SIZES[1]
    cam_a, bg = rt.scene_camera(0, W, H)
    cam_b = rt.camera_new((-4.0, 3.0, 9.0), (1.0, 0.5, 0.0), (0.0, 1.0, 0.0), 30.0, W / H, 0.05, 9.0, 0.0, 1.0)
    n_a = rt.primary_sky_tiles_host(soa, cam_a, W, H, K)[1]
    n_b = rt.primary_sky_tiles_host(soa, cam_b, W, H, K)[1]
    assert n_a > 0 and n_b > 0 and n_a != n_b
    off_a, _ = _render(rt, r, cam_a, bg, W, H, spp, 50, False)
    off_b, _ = _render(rt, r, cam_b, bg, W, H, spp, 50, False)
    r.upload(world)
    seq = [(cam_a, n_a, off_a, True), (cam_a, n_a, off_a, False), (cam_b, n_b, off_b, True), (cam_b, n_b, off_b, False),
           (cam_a, n_a, off_a, True)]
    for cam, n, ref, built in seq:
        img, st = _render(rt, r, cam, bg, W, H, spp, 50, True)
        assert (st.primary_build_ms > 0.0) == built and st.sky_tiles == n
        _same(img, ref, "camera change")
    r.upload(world)
    img, st = _render(rt, r, cam_a, bg, W, H, spp, 50, True)
    assert st.primary_build_ms > 0.0 and st.sky_tiles == n_a      # a new upload: dropped with the table
    _same(img, off_a, "after an upload")
    # without a table there is nothing to skip
    r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES, 0)
    try:
        img, st = _render(rt, r, cam_a, bg, W, H, spp, 50, True)
    finally:
        r.set_option(rt.RT_OPT_PRIMARY_CANDIDATES, 1)
    assert st.sky_tiles == 0 and st.primary_table_bytes == 0
    _same(img, off_a, "no table")


def test_the_option_is_additive_and_checked(rt, ctx):
    r, _, _ = ctx
    assert rt.RT_OPT_SKIP_SKY_TILES == 14 and r.get_option(rt.RT_OPT_SKIP_SKY_TILES) == 1
    for bad in (2, -1):
        with pytest.raises(rt.RTError):
            r.set_option(rt.RT_OPT_SKIP_SKY_TILES, bad)
    r.set_option(rt.RT_OPT_SKIP_SKY_TILES, 0)
    assert r.get_option(rt.RT_OPT_SKIP_SKY_TILES) == 0
    r.set_option(rt.RT_OPT_SKIP_SKY_TILES, 1)
