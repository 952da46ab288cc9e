"""The gather path (rt_render_gather, csrc/comm.cpp) held to rt_render on the one GPU: the slab
layout the library itself uses at N > 1, a tile order made for another frame, a rank whose
render fails, and the f32 mode. Every assertion is bit equality.

RCCL refuses two ranks on one device, so no N > 1 communicator is built here. What N > 1 adds to
the world-1 gather is the layout: rank r >= 1's slab and status trailer at r * slab_bytes of rank
0's buffer, and the element stride slab_bytes / esz — 192 n_max + 1 elements in f64, + 2 in f32,
because the 8-byte trailer rides in the stride — handed to the reorder kernel. The tests build
that buffer as the gather would land it: shard r rendered straight to byte r * slab_bytes of a
0xFF-filled (NaN in both formats) uint8 buffer, a zero trailer after it, then rt_tiles_assemble
with the library's stride, into a frame that sits between sentinel guards. The geometry comes
from tests/gather_reference.py, which tests/test_gather_layout.py holds csrc/comm_layout.hpp to.

Shapes (the smallest with each edge; random spheres at 4 spp): (160, 90) 20 x 12 tiles, the last
tile row cut; (40, 24) 15 tiles, at world 8 ranks hold 2 and 1; (67, 5) 9 x 1, ragged in both
axes; (9, 7) 2 tiles, at world 3 and 8 most ranks hold none. Larger sample counts appear only
where a buffer bound must be exceeded, and say why.
"""
import numpy as np
import pytest

from tests import gather_reference as gr

pytestmark = pytest.mark.gpu

SPP = 4
SHAPES = [(160, 90), (40, 24), (67, 5), (9, 7)]
WORLDS = [2, 3, 8]
ORDERS = ["raster", "reversed", "permuted"]
GUARD = 1024          # sentinel elements on each side of the assembled frame
SENTINEL = -12345.0   # no radiance is negative
MIB = 1 << 20


def tile_order(kind, n, seed=1234):
    if kind == "raster":
        return None
    if kind == "reversed":
        return np.arange(n, dtype=np.uint32)[::-1].copy()
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def _same(a, b, label):
    assert a.dtype == b.dtype and a.shape == b.shape, label
    same = a.view(np.uint8) == b.view(np.uint8)
    assert same.all(), f"{label}: {int((~same.reshape(-1, 3 * a.dtype.itemsize).all(axis=-1)).sum())} px differ"


@pytest.fixture(scope="module")
def spheres(rt, renderer):
    """The session's renderer with the random-spheres scene, in its default state; (renderer,
    ref(W, H, fmt, spp) -> the one-launch frame, rendered once per key and shared)."""
    renderer.upload(rt.World(1).build_scene(0))
    renderer.set_tile_order(None)
    cache = {}

    def ref(W, H, fmt, spp=SPP):
        key = (W, H, fmt, spp)
        if key not in cache:
            cam, bg = rt.scene_camera(0, W, H)
            img = renderer.render(cam, rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=fmt))
            img.setflags(write=False)
            cache[key] = img
        return cache[key]
    return renderer, ref


def gathered_frame(rt, r, scene, W, H, world, fmt, order, spp=SPP, **kw):
    """The N > 1 buffer built on the one GPU and reassembled by rt_tiles_assemble with the stride
    rt_render_gather passes. Returns (frame, the shard renders' stats); asserts what does not
    depend on a reference render: the frame equals gather_reference's reassembly of the downloaded
    bytes, both guards and the gathered buffer are untouched, every trailer is zero, and a rank
    with no tile wrote nothing. The context's tile order is the caller's to set (and reset)."""
    import torch
    cam, bg = rt.scene_camera(scene, W, H)
    esz = 8 if fmt == rt.RT_OUT_F64 else 4
    dt = torch.float64 if esz == 8 else torch.float32
    g = gr.slab_geometry(W, H, world, esz)
    dev = torch.device("cuda", 0)
    gathered = torch.full((g["gathered_bytes"],), 0xFF, dtype=torch.uint8, device=dev)
    buf = torch.full((GUARD + H * W * 3 + GUARD,), SENTINEL, dtype=dt, device=dev)
    stats = []
    stream = torch.cuda.Stream(dev)
    stream.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(stream):
        for q in range(world):
            p = rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=fmt, row_begin=q, row_stride=world, tile_shard=1, **kw)
            r.render_device(cam, p, gathered.data_ptr() + q * g["slab_bytes"], stream.cuda_stream)   # RT_OK, or it raises
            st = r.stats()
            stats.append((st.schedule, st.ring_bytes > 0, st.n_batches))
            gathered[g["status_at"][q]:g["status_at"][q] + 8] = 0
        before = gathered.clone()
        p = rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=fmt)
        r.assemble_device(gathered.data_ptr(), g["stride_elems"], world, p, buf.data_ptr() + GUARD * esz,
                          stream.cuda_stream)
    stream.synchronize()
    label = (W, H, world, esz)
    assert torch.equal(gathered, before), label
    host_buf = buf.cpu().numpy()
    assert (host_buf[:GUARD] == SENTINEL).all() and (host_buf[-GUARD:] == SENTINEL).all(), label
    frame = host_buf[GUARD:-GUARD].reshape(H, W, 3).copy()
    raw = gathered.cpu().numpy()
    assert gr.statuses(raw, W, H, world, esz) == [0] * world, label
    for q in range(world):
        if g["n_mine"][q] == 0:   # an empty shard: its slab is still the 0xFF fill
            assert (raw[q * g["slab_bytes"]:g["status_at"][q]] == 0xFF).all(), label
    total = gr.n_tiles(W, H)
    _same(frame, gr.reassemble(raw, W, H, world, esz, order if order is not None else np.arange(total), fill=np.nan),
          f"{label} against gather_reference")
    return frame, stats


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_library_layout_reassembles_to_rt_render(rt, spheres, shape, world):
    """3 orders x 2 formats per (shape, world): the reassembled frame is rt_render's one-launch frame."""
    r, ref = spheres
    W, H = shape
    try:
        for kind in ORDERS:
            order = tile_order(kind, gr.n_tiles(W, H))
            r.set_tile_order(order)
            for fmt in (rt.RT_OUT_F64, rt.RT_OUT_F32):
                frame, _ = gathered_frame(rt, r, 0, W, H, world, fmt, order)
                _same(frame, ref(W, H, fmt), f"{shape} world {world} {kind} fmt {fmt}")
    finally:
        r.set_tile_order(None)


def test_library_layout_final_scene(rt, spheres):
    """The final scene (BVH, media, textures, motion blur) once, at (40, 24): world 3 and 8, a permuted order."""
    r, _ = spheres
    W, H = 40, 24
    cam, bg = rt.scene_camera(7, W, H)
    try:
        r.upload(rt.World(1).build_scene(7))
        order = tile_order("permuted", gr.n_tiles(W, H))
        for fmt in (rt.RT_OUT_F64, rt.RT_OUT_F32):
            r.set_tile_order(None)
            want = r.render(cam, rt.Renderer.params(W, H, SPP, 50, bg, 1, out_format=fmt))
            r.set_tile_order(order)
            for world in (3, 8):
                frame, _ = gathered_frame(rt, r, 7, W, H, world, fmt, order)
                _same(frame, want, f"final scene world {world} fmt {fmt}")
    finally:
        r.set_tile_order(None)
        r.upload(rt.World(1).build_scene(0))


# ---- a tile order made for another frame ------------------------------------------------------------
def _stale_order_checks(rt, r, ref, gather_host, gather_device):
    """The context holds a (160, 90) order. gather_host(cam, p, out) / gather_device(cam, p, ptr)
    run one flavour of the gather; both refuse a frame with more tiles and one with fewer before
    anything is enqueued, leave the frame alone, and go on working at (160, 90)."""
    import torch
    dev = torch.device("cuda", 0)
    for W, H in ((168, 96), (80, 48)):   # 21 x 12 = 252 tiles, 10 x 6 = 60; the order has 240
        cam, bg = rt.scene_camera(0, W, H)
        out = np.full((H, W, 3), np.nan, dtype=np.float64)
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID.*tile order is for another frame"):
            gather_host(cam, rt.Renderer.params(W, H, SPP, 50, bg, 1, out_format=rt.RT_OUT_F64), out)
        assert np.isnan(out).all(), (W, H)
        frame = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device=dev)
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID.*tile order is for another frame"):
            gather_device(cam, rt.Renderer.params(W, H, SPP, 50, bg, 1, out_format=rt.RT_OUT_F64), frame.data_ptr())
        torch.cuda.synchronize(dev)
        assert bool(torch.isnan(frame).all()), (W, H)
    W, H = 160, 90
    cam, bg = rt.scene_camera(0, W, H)
    out = np.full((H, W, 3), np.nan, dtype=np.float64)
    gather_host(cam, rt.Renderer.params(W, H, SPP, 50, bg, 1, out_format=rt.RT_OUT_F64), out)
    _same(out, ref(W, H, rt.RT_OUT_F64), "the order's own frame, right after")
    frame = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device=dev)
    gather_device(cam, rt.Renderer.params(W, H, SPP, 50, bg, 1, out_format=rt.RT_OUT_F64), frame.data_ptr())
    torch.cuda.synchronize(dev)
    _same(frame.cpu().numpy(), ref(W, H, rt.RT_OUT_F64), "the order's own frame, device output")
    r.set_tile_order(None)
    W, H = 168, 96
    cam, bg = rt.scene_camera(0, W, H)
    out = np.full((H, W, 3), np.nan, dtype=np.float64)
    gather_host(cam, rt.Renderer.params(W, H, SPP, 50, bg, 1, out_format=rt.RT_OUT_F64), out)
    _same(out, ref(W, H, rt.RT_OUT_F64), "raster order again")


@pytest.mark.parametrize("entry", ["gather", "gather_all"])
def test_stale_tile_order_is_refused_before_anything_is_enqueued(rt, spheres, entry):
    """rt_comm_tile_order at (160, 90), then a gather at another frame size: RT_ERR_INVALID from
    every rank before anything is enqueued (the reorder kernel would read order[pos] up to the
    new frame's tile count). World 1, RT_OPT_COMM_DIRECT 0: the shard, gather and reorder path."""
    r, ref = spheres
    cam, bg = rt.scene_camera(0, 160, 90)
    p0 = rt.Renderer.params(160, 90, SPP, 50, bg, 1, out_format=rt.RT_OUT_F64)
    comms = []
    try:
        r.set_option(rt.RT_OPT_COMM_DIRECT, 0)
        if entry == "gather":
            comms = [rt.Comm(r, 0, 1, rt.Comm.unique_id())]
            comms[0].tile_order(cam, p0, 4)

            def host(c, p, out):
                return comms[0].render_gather(c, p, out=out)

            def device(c, p, ptr):
                return comms[0].render_gather_device(c, p, ptr)
        else:
            comms = rt.Comm.init_all([r])
            rt.tile_order_all(comms, cam, p0, 4)

            def host(c, p, out):
                return rt.render_gather_all(comms, c, p, out=out)

            def device(c, p, ptr):
                return rt.render_gather_all_device(comms, c, p, ptr)
        assert comms[0].stats().tile_order == 1
        _stale_order_checks(rt, r, ref, host, device)
    finally:
        for c in comms:
            c.close()
        r.set_tile_order(None)
        r.set_option(rt.RT_OPT_COMM_DIRECT, 1)


# ---- a rank whose render fails -------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [0, 1])
def test_failed_rank_reports_through_the_trailer(rt, direct):
    """A context with no scene: the shard render returns RT_ERR_NO_SCENE, the rank still takes
    part in the gather with -rc in its trailer, and rank 0 counts it (stats.peer_failed). No
    kernel runs on uninitialised indices: the unrendered slab is only copied. With
    RT_OPT_COMM_DIRECT 1 there is no slab: the error is reported, peer_failed stays 0."""
    import torch
    W, H = 40, 24
    dev = torch.device("cuda", 0)
    cam, bg = rt.scene_camera(0, W, H)

    def params():
        return rt.Renderer.params(W, H, SPP, 50, bg, 1, out_format=rt.RT_OUT_F64)
    r = rt.Renderer(0)
    comm = None
    try:
        r.set_option(rt.RT_OPT_COMM_DIRECT, direct)
        comm = rt.Comm(r, 0, 1, rt.Comm.unique_id())
        with pytest.raises(rt.RTError, match="RT_ERR_NO_SCENE"):
            comm.render_gather(cam, params())
        assert comm.stats().peer_failed == (0 if direct else 1)
        assert comm.stats().peer_failed == (0 if direct else 1)   # a second read still returns
        frame = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device=dev)
        with pytest.raises(rt.RTError, match="RT_ERR_NO_SCENE"):
            comm.render_gather_device(cam, params(), frame.data_ptr())
        st = comm.stats()   # (waits for the enqueued gather)
        assert st.peer_failed == (0 if direct else 1)
        assert comm.stats().peer_failed == st.peer_failed

        r.upload(rt.World(1).build_scene(0))
        want = r.render(cam, params())
        _same(comm.render_gather(cam, params()), want, f"direct {direct}, host output")
        st = comm.stats()
        assert st.peer_failed == 0 and st.tiles == 15
        assert st.slab_bytes == (0 if direct else gr.slab_geometry(W, H, 1, 8)["slab_bytes"])
        frame.fill_(float("nan"))
        comm.render_gather_device(cam, params(), frame.data_ptr())
        assert comm.stats().peer_failed == 0
        torch.cuda.synchronize(dev)
        _same(frame.cpu().numpy(), want, f"direct {direct}, device output")
    finally:
        if comm is not None:
            comm.close()
        r.close()


# ---- the f32 mode ---------------------------------------------------------------------------------------
# (schedule, RT_OPT_POOL_RING, spp_chunk): the four trace kernels. POOL's ring needs work blocks of
# exactly one chunk: spp_chunk 16 at 4 spp is one 4-sample chunk, which a small frame's blocks keep.
KERNELS = {"pool_buffer": ("POOL", 0, 0), "pool_ring": ("POOL", 2, 16), "items": ("ITEMS", 1, 0), "chunks": ("CHUNKS", 1, 0)}


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_f32_mode_one_kernel_one_frame(rt, spheres, kernel):
    """RT_PREC_F32 under each forced trace kernel: the world-1 gather (raster and permuted order)
    and the world-3 reassembly are rt_render's frame bit for bit, and rt_stats shows the shards
    and the whole frame ran that kernel. POOL's buffer in >= 3 batches has the one-batch bits."""
    r, _ = spheres
    W, H = 160, 90
    sched_name, ring, spp_chunk = KERNELS[kernel]
    sched = getattr(rt, "RT_SCHED_" + sched_name)
    want_kernel = (sched, kernel == "pool_ring")
    cam, bg = rt.scene_camera(0, W, H)
    bound = r.get_option(rt.RT_OPT_TRACE_BUF_BYTES)
    order = tile_order("permuted", gr.n_tiles(W, H))
    comm = None

    def params(fmt, spp=SPP):
        return rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=fmt, spp_chunk=spp_chunk)

    def kernel_of(st):
        return (st.schedule, st.ring_bytes > 0)
    try:
        r.set_precision(rt.RT_PREC_F32)
        r.set_schedule(sched)
        r.set_option(rt.RT_OPT_POOL_RING, ring)
        r.set_option(rt.RT_OPT_COMM_DIRECT, 0)
        want = {}
        for fmt in (rt.RT_OUT_F64, rt.RT_OUT_F32):
            want[fmt] = r.render(cam, params(fmt))
            st = r.stats()
            assert st.precision == rt.RT_PREC_F32 and kernel_of(st) == want_kernel and st.n_batches == 1, kernel
        comm = rt.Comm(r, 0, 1, rt.Comm.unique_id())
        for o in (None, order):
            r.set_tile_order(o)
            got = comm.render_gather(cam, params(rt.RT_OUT_F64))
            assert kernel_of(r.stats()) == want_kernel and comm.stats().slab_bytes > 0, kernel
            _same(got, want[rt.RT_OUT_F64], f"{kernel}: world-1 gather, order {'raster' if o is None else 'permuted'}")
        for fmt in (rt.RT_OUT_F64, rt.RT_OUT_F32):   # (the permuted order is still set)
            frame, stats = gathered_frame(rt, r, 0, W, H, 3, fmt, order, spp_chunk=spp_chunk)
            assert [s[:2] for s in stats] == [want_kernel] * 3, (kernel, stats)
            _same(frame, want[fmt], f"{kernel}: world-3 reassembly, fmt {fmt}")
        if kernel == "pool_buffer":
            # 12 spp: an f32 sample of the 160 x 96 tiled frame is 184,320 B, the smallest bound (1 MiB)
            # holds 5 of them: 3 batches (the spheres variant's large workgroups do not overlap batches)
            r.set_tile_order(None)
            one = r.render(cam, params(rt.RT_OUT_F64, 12))
            assert kernel_of(r.stats()) == want_kernel and r.stats().n_batches == 1
            r.set_option(rt.RT_OPT_TRACE_BUF_BYTES, MIB)
            batched = r.render(cam, params(rt.RT_OUT_F64, 12))
            st = r.stats()
            assert kernel_of(st) == want_kernel and st.n_batches >= 3, st.n_batches
            _same(batched, one, "pool_buffer: 3 batches against one")
    finally:
        if comm is not None:
            comm.close()
        r.set_tile_order(None)
        r.set_precision(rt.RT_PREC_F64)
        r.set_schedule(rt.RT_SCHED_AUTO)
        r.set_option(rt.RT_OPT_POOL_RING, 1)
        r.set_option(rt.RT_OPT_COMM_DIRECT, 1)
        r.set_option(rt.RT_OPT_TRACE_BUF_BYTES, bound)


def test_auto_split_shards_pool_frame_items_same_f64_bits(rt, spheres):
    """RT_SCHED_AUTO, f64: a bound at which the world-3 shards take POOL and the whole frame
    ITEMS. AUTO takes POOL while samples x tiled pixels x 24 B <= 4 x the bound. Under the smallest
    bound (1 MiB) with the ring off, (160, 90) at 12 spp is 12 x 160 x 96 x 24 = 4,423,680 B >
    4 MiB for the frame and a third of it for an 80-tile shard. In f64 the bits are the same."""
    r, ref = spheres
    W, H, spp = 160, 90, 12
    cam, bg = rt.scene_camera(0, W, H)
    bound = r.get_option(rt.RT_OPT_TRACE_BUF_BYTES)
    try:
        r.set_option(rt.RT_OPT_POOL_RING, 0)
        r.set_option(rt.RT_OPT_TRACE_BUF_BYTES, MIB)
        whole = r.render(cam, rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=rt.RT_OUT_F64))
        assert r.stats().schedule == rt.RT_SCHED_ITEMS
        frame, stats = gathered_frame(rt, r, 0, W, H, 3, rt.RT_OUT_F64, None, spp=spp)
        assert [s[0] for s in stats] == [rt.RT_SCHED_POOL] * 3, stats
        _same(frame, whole, "POOL shards against the ITEMS frame")
        r.set_option(rt.RT_OPT_TRACE_BUF_BYTES, bound)
        r.set_option(rt.RT_OPT_POOL_RING, 1)
        _same(whole, ref(W, H, rt.RT_OUT_F64, spp), "the bounded ITEMS frame against the default render")
    finally:
        r.set_option(rt.RT_OPT_POOL_RING, 1)
        r.set_option(rt.RT_OPT_TRACE_BUF_BYTES, bound)
