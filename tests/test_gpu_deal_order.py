"""The whole-frame deal order (RT_OPT_AUTO_DEAL_ORDER, rt_last_deal_order; csrc/deal_cache.cpp):
the first render of a (scene upload, camera, frame) measures each tile's cost in the product
kernel, the second builds the cost order from it, later ones reuse it.

Only the order in which work blocks are handed out changes, never a pixel's bits: under every
pool schedule, precision, across buffer batches, through rt_render_gather and rt_accum_add the
measuring render, the ordered renders and a render with the option off are the same frame.

The frame is the random scene at 156x92 (20 x 12 tiles, the right and the top ones ragged),
40 spp (with blocks of 16 samples the last sample group is partial), depth 50.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP, TILES = 156, 92, 40, 240

# test_measured_order_puts_the_cheap_tiles_last: the share of the count pass's cheapest quarter of
# tiles (60 of 240) that the measured order puts in its last quarter. DESIGN.md §6.1 ("the deal
# order's quality"): five renders on an MI355X gave 0.900, 0.900, 0.867, 0.900, 0.883 (52 .. 54 of 60 tiles); an
# order that knew nothing would give 0.25. The bound is the lowest of the five less twice their
# spread.
CHEAP_SHARE_MIN = 0.80


@pytest.fixture(scope="module")
def ctx(rt):
    """A context of this module's own (the option and the cache are per context) and the random scene."""
    r = rt.Renderer(0)
    world = rt.World(1).build_scene(0)
    cam, bg = rt.scene_camera(0, W, H)
    r.upload(world)
    yield r, world, cam, bg
    r.close()


def _params(rt, bg, spp=SPP, w=W, h=H, max_depth=50, **kw):
    return rt.Renderer.params(w, h, spp, max_depth, bg, 1, out_format=rt.RT_OUT_F64, **kw)


def _is_order(o, n=TILES):
    return len(o) == n and np.array_equal(np.sort(o), np.arange(n))


def _three_and_off(rt, r, world, frame):
    """frame() three times under option 1 on a fresh key, once under option 0: the four frames, after
    checking that the first ran in raster order, the next two in one order, the last in raster order."""
    r.upload(world)   # a new upload drops the entry
    r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 1)
    try:
        a = frame()
        assert len(r.deal_order()) == 0
        b = frame()
        o = r.deal_order()
        assert _is_order(o)
        c = frame()
        assert np.array_equal(r.deal_order(), o)
        r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
        d = frame()
        assert len(r.deal_order()) == 0
    finally:
        r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 1)
    return a, b, c, d


def _all_equal(frames):
    assert all(f.shape == frames[0].shape and np.array_equal(f, frames[0]) for f in frames[1:])
    assert np.isfinite(frames[0]).all() and frames[0].max() > 0


SCHEDULES = {
    # name: (schedule, RT_OPT_POOL_RING, spp_chunk)
    "pool_buffer": ("RT_SCHED_POOL", 0, 0),
    "pool_ring": ("RT_SCHED_POOL", 2, 16),   # the ring takes blocks of one chunk
    "items": ("RT_SCHED_ITEMS", 1, 0),
}


@pytest.mark.parametrize("precision", ["RT_PREC_F64", "RT_PREC_F32"])
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_ordered_frames_are_bit_identical(rt, ctx, name, precision):
    r, world, cam, bg = ctx
    sched, ring, chunk = SCHEDULES[name]
    r.set_schedule(getattr(rt, sched))
    r.set_precision(getattr(rt, precision))
    r.set_option(rt.RT_OPT_POOL_RING, ring)
    r.set_option(rt.RT_OPT_BLOCK_SAMPLES, 16)
    try:
        def frame():
            f = r.render(cam, _params(rt, bg, spp_chunk=chunk))
            st = r.stats()
            assert st.schedule == getattr(rt, sched) and (st.ring_bytes > 0) == (name == "pool_ring")
            assert st.n_batches == 1
            return f
        _all_equal(_three_and_off(rt, r, world, frame))
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
        r.set_precision(rt.RT_PREC_F64)
        r.set_option(rt.RT_OPT_POOL_RING, 1)
        r.set_option(rt.RT_OPT_BLOCK_SAMPLES, 0)


def test_every_buffer_batch_takes_the_order(rt, ctx):
    r, world, cam, bg = ctx
    r.set_schedule(rt.RT_SCHED_POOL)
    r.set_option(rt.RT_OPT_POOL_RING, 0)
    r.set_option(rt.RT_OPT_BLOCK_SAMPLES, 16)
    try:
        one = r.render(cam, _params(rt, bg))
        assert r.stats().n_batches == 1
        r.set_option(rt.RT_OPT_TRACE_BUF_BYTES, 4 << 20)   # 368,640 B of records per sample: ~11 samples per batch

        def frame():
            f = r.render(cam, _params(rt, bg))
            assert r.stats().n_batches >= 3
            return f
        _all_equal([one, *_three_and_off(rt, r, world, frame)])
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
        for key, v in ((rt.RT_OPT_POOL_RING, 1), (rt.RT_OPT_BLOCK_SAMPLES, 0), (rt.RT_OPT_TRACE_BUF_BYTES, 0)):
            r.set_option(key, v)


def test_render_gather_of_one_rank_stays_direct_and_takes_the_order(rt, ctx):
    r, world, cam, bg = ctx
    ref = r.render(cam, _params(rt, bg))
    comm = rt.Comm(r, 0, 1, rt.Comm.unique_id())
    try:
        assert r.get_option(rt.RT_OPT_COMM_DIRECT) == 1

        def frame():
            f = comm.render_gather(cam, _params(rt, bg))
            assert comm.stats().slab_bytes == 0
            return f
        _all_equal([ref, *_three_and_off(rt, r, world, frame)])
    finally:
        comm.close()


def test_accumulated_batches_take_the_order(rt, ctx):
    """rt_accum_add in batches of 16 + 16 + 8 samples (chunks of 8): the second batch builds the
    order, the third reuses it; the sums are the one render's."""
    r, world, cam, bg = ctx
    p = _params(rt, bg, spp_chunk=8)
    one = r.render(cam, p)
    r.upload(world)
    acc = rt.Accumulator(r, p)
    try:
        dealt = []
        for n in (16, 16, 8):
            acc.add(cam, p, n)
            dealt.append(len(r.deal_order()))
        assert dealt == [0, TILES, TILES]
        got = acc.resolve(out_format=rt.RT_OUT_F64)
    finally:
        acc.close()
    assert np.array_equal(got, one)


def test_the_final_scene_variant_keeps_raster_order(rt):
    """The other kernel family (the final scene's variant: block state in a VGPR's lanes, the
    select form of the block mapping) has the deal order compiled out (trace_kernel.hpp,
    deal_variant): its renders stay raster under every option, per-sample buffer and ring."""
    w, h, spp = 96, 64, 20
    r = rt.Renderer(0)
    try:
        world = rt.World(1).build_scene(7)
        cam, bg = rt.scene_camera(7, w, h)
        r.set_schedule(rt.RT_SCHED_POOL)
        r.set_option(rt.RT_OPT_BLOCK_SAMPLES, 16)
        frames = []
        for ring in (0, 2):
            r.set_option(rt.RT_OPT_POOL_RING, ring)
            r.upload(world)
            for i in range(3):
                frames.append(r.render(cam, _params(rt, bg, spp=spp, w=w, h=h, spp_chunk=16)))
                assert (r.stats().ring_bytes > 0) == (ring == 2)
                assert len(r.deal_order()) == 0
        r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
        frames.append(r.render(cam, _params(rt, bg, spp=spp, w=w, h=h, spp_chunk=16)))
        assert len(r.deal_order()) == 0
        _all_equal(frames)
    finally:
        r.close()


def test_deal_order_state(rt, ctx):
    r, world, cam, bg = ctx
    cam2, _ = rt.scene_camera(0, W, H)
    cam2.origin[0] += 0.25
    frame = lambda c=cam, **kw: r.render(c, _params(rt, bg, spp=4, **kw))
    r.upload(world)
    assert r.get_option(rt.RT_OPT_AUTO_DEAL_ORDER) == 1
    try:
        frame()
        assert len(r.deal_order()) == 0                     # the first render measures
        frame()
        o = r.deal_order()
        assert _is_order(o)                                 # the second is ordered
        r.render(cam, _params(rt, bg, spp=9, max_depth=7))
        assert np.array_equal(r.deal_order(), o)            # not keyed by spp or depth
        # a tile shard under a context order in between: its own order, ours untouched
        ctx_order = np.arange(TILES)[::-1].copy()
        r.set_tile_order(ctx_order)
        whole = frame()
        assert np.array_equal(r.deal_order(), o)
        slabs = [frame(row_begin=k, row_stride=2, tile_shard=1) for k in range(2)]
        assert len(r.deal_order()) == 0
        assert np.array_equal(rt.assemble_tiles(slabs, W, H, 2, order=ctx_order), whole)
        r.set_tile_order(None)
        frame(count_work=1)
        assert len(r.deal_order()) == 0 and len(r.tile_costs()) == TILES
        frame()
        assert np.array_equal(r.deal_order(), o)
        # another camera, another width, a new upload: raster again, then an order of their own
        frame(cam2)
        assert len(r.deal_order()) == 0
        frame(cam2)
        assert _is_order(r.deal_order())
        frame(w=148)
        assert len(r.deal_order()) == 0
        frame(w=148)
        assert _is_order(r.deal_order(), 19 * 12)
        frame()
        assert len(r.deal_order()) == 0
        frame()
        assert _is_order(r.deal_order())
        r.upload(world)
        assert len(r.deal_order()) == 0                     # the order went with the upload
        frame()
        assert len(r.deal_order()) == 0
        # option 0 and option 2 never order
        for mode in (0, 2):
            r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, mode)
            for _ in range(3):
                frame()
                assert len(r.deal_order()) == 0
        with pytest.raises(RuntimeError):
            r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 3)
    finally:
        r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 1)
        r.set_tile_order(None)


def cheap_share(costs, order):
    """Of the quarter of tiles with the lowest reference costs, the share in the order's last quarter."""
    q = len(costs) // 4
    cheap = set(np.argsort(costs, kind="stable")[:q].tolist())
    return len(cheap & set(np.asarray(order)[-q:].tolist())) / q


def test_measured_order_puts_the_cheap_tiles_last(rt, ctx):
    """Against the count pass (count_work at the same spp, rt_last_tile_costs: per-lane cycles per
    tile), the reference the multi-GPU order is built from."""
    r, world, cam, bg = ctx
    r.set_schedule(rt.RT_SCHED_POOL)
    try:
        r.upload(world)
        r.render(cam, _params(rt, bg, count_work=1))
        costs = r.tile_costs()
        assert len(costs) == TILES and (costs > 0).all()
        r.render(cam, _params(rt, bg))
        r.render(cam, _params(rt, bg))
        order = r.deal_order()
        assert _is_order(order)
        share = cheap_share(costs, order)
        print("cheapest quarter in the order's last quarter: %.3f (bound %.2f)" % (share, CHEAP_SHARE_MIN))
        assert share >= CHEAP_SHARE_MIN
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
