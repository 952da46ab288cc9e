"""Wave-wide sample starts in the spheres variant's per-sample pool (csrc/launch_shapes.hpp
RT_STAGE_SEEDS; csrc/trace_device.hpp trace_pool's CfgStage instantiations): when a wave takes
units from the start of a sample row of its work block, it seeds and jitters all of the tile's
pixels for that sample at once into LDS slots, and a lane that takes a unit reads its slot.

Every lane's stream is still Philox(seed, pixel, sample) followed by its own draws in its own
order, so no bit may change. The chunk schedule (RT_SCHED_CHUNKS, trace_chunks) never enters
trace_pool and seeds per lane: it is the in-library reference, and every comparison with it is
exact. Scene 0 (the random spheres, the only scene of the staged variant) at depth 8: full tiles
only, partial tiles on both axes, and a single partial tile (nvalid = 35), at sample counts that
make one row, part of a block, whole blocks and a short last block.
"""
import numpy as np
import pytest

from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu

DEPTH = 8
SIZES = [(64, 48), (20, 12), (7, 5)]
SPPS = [1, 5, 16, 17, 40]
BLOCKS = [0, 4, 8]


@pytest.fixture(scope="module")
def ctx(rt):
    """A context of this module's own with the random scene uploaded, the deal order off (its own test turns it on)."""
    r = rt.Renderer(0)
    world = rt.World(1).build_scene(0)
    r.upload(world)
    r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
    yield r, world
    r.close()


def _render(rt, r, W, H, spp, sched, ring=0, block=0, spp_chunk=0, **kw):
    cam, bg = rt.scene_camera(0, W, H)
    r.set_schedule(sched)
    r.set_option(rt.RT_OPT_POOL_RING, ring)
    r.set_option(rt.RT_OPT_BLOCK_SAMPLES, block)
    try:
        img = r.render(cam, rt.Renderer.params(W, H, spp, DEPTH, bg, 1, out_format=rt.RT_OUT_F64, spp_chunk=spp_chunk, **kw))
        st = r.stats()
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
        r.set_option(rt.RT_OPT_POOL_RING, 1)
        r.set_option(rt.RT_OPT_BLOCK_SAMPLES, 0)
    assert st.schedule == sched
    return img, st


_REF = {}


def _chunks(rt, r, W, H, spp, spp_chunk=0, **kw):
    """The chunk schedule's frame: rendered once per configuration, shared and left unchanged."""
    key = (W, H, spp, spp_chunk, tuple(sorted(kw.items())))
    if key not in _REF:
        img, _ = _render(rt, r, W, H, spp, rt.RT_SCHED_CHUNKS, spp_chunk=spp_chunk, **kw)
        assert np.isfinite(img).all() and img.max() > 0
        img.setflags(write=False)
        _REF[key] = img
    return _REF[key]


@pytest.mark.parametrize("ring", [0, 2], ids=["buffer", "ring"])
@pytest.mark.parametrize("W,H", SIZES)
def test_pool_equals_chunks(rt, ctx, W, H, ring):
    """POOL against CHUNKS for every spp x block_samples of the module: exact. The ring takes blocks
    of exactly one chunk, so its cases with blocks of 4 and 8 samples set chunks of 4 and 8 too, both
    cut to spp where that is less (the automatic blocks of these small frames are one automatic
    chunk); the buffer form keeps the automatic chunks, so its blocks of 4 and 8 hold several chunks
    or cut one."""
    r, _ = ctx
    for spp in SPPS:
        for block in BLOCKS:
            chunk = min(block, spp) if ring and block else 0
            block = chunk if ring and block else block
            got, st = _render(rt, r, W, H, spp, rt.RT_SCHED_POOL, ring=ring, block=block, spp_chunk=chunk)
            assert (st.ring_bytes > 0) == (ring == 2), (spp, block)
            ref = _chunks(rt, r, W, H, spp, spp_chunk=chunk)
            assert np.array_equal(got, ref), "%dx%dx%d block %d ring %d: %d px differ" % (
                W, H, spp, block, ring, int((got != ref).any(axis=-1).sum()))


@pytest.mark.parametrize("ring", [0, 2], ids=["buffer", "ring"])
def test_tile_shards_assemble_to_the_whole_frame(rt, ctx, ring):
    r, _ = ctx
    W, H, spp = 20, 12, 17   # 3 x 2 tiles, the right column and the top row partial
    whole = _chunks(rt, r, W, H, spp)
    slabs = [_render(rt, r, W, H, spp, rt.RT_SCHED_POOL, ring=ring, row_begin=t, row_stride=3, tile_shard=1)[0]
             for t in range(3)]
    assert np.array_equal(rt.assemble_tiles(slabs, W, H, 3), whole)


def test_ordered_deal_equals_the_first_render(rt, ctx):
    """The automatic deal order: the first render measures in raster order, the second is dealt
    through the ordered table; same frame, and the chunk schedule's."""
    r, world = ctx
    W, H, spp = 64, 48, 17
    cam, bg = rt.scene_camera(0, W, H)
    p = rt.Renderer.params(W, H, spp, DEPTH, bg, 1, out_format=rt.RT_OUT_F64)
    ref = _chunks(rt, r, W, H, spp)
    r.upload(world)   # a new upload drops any order
    r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 1)
    r.set_schedule(rt.RT_SCHED_POOL)
    try:
        first = r.render(cam, p)
        assert len(r.deal_order()) == 0
        second = r.render(cam, p)
        assert len(r.deal_order()) == 8 * 6
    finally:
        r.set_schedule(rt.RT_SCHED_AUTO)
        r.set_option(rt.RT_OPT_AUTO_DEAL_ORDER, 0)
    assert np.array_equal(second, first) and np.array_equal(first, ref)


def _accumulated(rt, r, W, H, spp, chunk, sched, block, pieces):
    cam, bg = rt.scene_camera(0, W, H)
    p = rt.Renderer.params(W, H, spp, DEPTH, bg, 1, out_format=rt.RT_OUT_F64, spp_chunk=chunk)
    r.set_schedule(sched)
    r.set_option(rt.RT_OPT_BLOCK_SAMPLES, block)
    acc = r.accumulator(p)
    try:
        for n in pieces:
            acc.add(cam, p, n)
        return acc.resolve(out_format=rt.RT_OUT_F64)
    finally:
        acc.close()
        r.set_schedule(rt.RT_SCHED_AUTO)
        r.set_option(rt.RT_OPT_BLOCK_SAMPLES, 0)


def test_accumulated_17_plus_23_equals_one_render(rt, ctx):
    """An accumulator fed 40 samples as 17 + 23 (sample_begin != 0 in the second launch).

    rt_accum_add starts its chunks at the first sample it is given, so a piece that ends inside a
    chunk regroups the sum: with the automatic chunks of 3 (17 = 5 x 3 + 2) the accumulator's frame
    differs from one render's in the last bits on every schedule, the chunk schedule and the
    parent commit included (the project's own accumulator tests split on chunk boundaries). So:
      - chunks of 1, where the order of additions is the one render's whatever the split: the
        accumulator equals one 40-sample render exactly, with work blocks of 8 samples so that
        the split at 17 falls inside a block, and rows of the second launch start at sample 17;
      - chunks of 3, the split inside a chunk: the accumulator under POOL equals the accumulator
        under CHUNKS fed the same pieces exactly (its distance from the one render is printed).
    """
    r, _ = ctx
    W, H, spp = 20, 12, 40
    one, _ = _render(rt, r, W, H, spp, rt.RT_SCHED_POOL, spp_chunk=1)
    assert np.array_equal(one, _chunks(rt, r, W, H, spp, spp_chunk=1))
    for block in (0, 8):
        got = _accumulated(rt, r, W, H, spp, 1, rt.RT_SCHED_POOL, block, (17, 23))
        assert np.array_equal(got, one), "chunks of 1, blocks of %d" % block
    pool3 = _accumulated(rt, r, W, H, spp, 3, rt.RT_SCHED_POOL, 0, (17, 23))
    chunks3 = _accumulated(rt, r, W, H, spp, 3, rt.RT_SCHED_CHUNKS, 0, (17, 23))
    print("chunks of 3, 17 + 23: max |accumulator - one render| = %.3e" %
          float(np.abs(pool3 - _chunks(rt, r, W, H, spp, spp_chunk=3)).max()))
    assert np.array_equal(pool3, chunks3)


def test_against_the_oracle(rt, ctx):
    """20x12x5 against the CPU oracle, at the tolerance tests/test_gpu_parity.py uses for scene 0."""
    r, _ = ctx
    W, H, spp = 20, 12, 5
    got, _ = _render(rt, r, W, H, spp, rt.RT_SCHED_POOL)
    ref = ob.render(0, W, H, spp, DEPTH)
    d = np.abs(got - ref)
    assert np.isfinite(got).all()
    assert float(d.max()) <= 1e-3                                  # LINF
    assert not (d > 1e-9 * np.maximum(1.0, np.abs(ref))).any()     # REL: path identity
