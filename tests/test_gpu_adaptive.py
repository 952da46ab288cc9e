"""rt_render_adaptive: noise-driven sample counts per 8x8 tile (include/rt/rt_abi.h).

Every draw is keyed by (pixel, sample), so the result is held to exact references: with the
threshold off the frame is rt_render's bit for bit; a tile that stopped at n samples holds
rt_render's pixels at spp = n (same chunk) bit for bit, and the oracle's within the usual parity
bound; the stop counts themselves are predicted from oracle-derived samples and a numpy
restatement of the criterion (tests/adaptive_reference.py), never from the library.
"""
import numpy as np
import pytest

from tests import adaptive_reference as ar
from tests import oracle_binding as ob

pytestmark = pytest.mark.gpu

LINF = 1e-3   # the project's parity bound on the linear mean radiance
REL = 1e-9    # path identity


def _setup(rt, renderer, scene, W, H):
    renderer.upload(rt.World(1).build_scene(scene))
    return rt.scene_camera(scene, W, H)


def _params(rt, bg, W, H, spp, chunk=0, **kw):
    return rt.Renderer.params(W, H, spp, 50, bg, 1, spp_chunk=chunk, out_format=rt.RT_OUT_F64, **kw)


def _passes(spp, min_r, step_r):
    return 1 + -(-(spp - min(min_r, spp)) // step_r)


@pytest.mark.parametrize("scene,W,H,spp,chunk,min_spp,step_spp",
                         [(0, 37, 21, 40, 4, 8, 8), (5, 32, 32, 17, 0, 4, 6), (7, 72, 40, 20, 0, 6, 3)])
def test_threshold_zero_is_rt_render(rt, renderer, scene, W, H, spp, chunk, min_spp, step_spp):
    """threshold 0 never stops early: rt_render's frame at p->spp bit for bit, every tile at spp."""
    cam, bg = _setup(rt, renderer, scene, W, H)
    full = renderer.render(cam, _params(rt, bg, W, H, spp, chunk))
    mean, tile_spp, tile_error, se = renderer.render_adaptive(cam, _params(rt, bg, W, H, spp, chunk), min_spp,
                                                               step_spp, 0.0)
    assert np.array_equal(mean, full)
    assert (tile_spp == spp).all()
    assert np.isfinite(tile_error).all() and np.isfinite(se).all() and se.max() > 0
    st = renderer.adaptive_stats()
    c = st.spp_chunk
    assert c == (chunk or min(16, max(1, (spp + 15) // 16)))
    assert st.min_spp == -(-min_spp // c) * c and st.step_spp == -(-step_spp // c) * c
    assert st.passes == _passes(spp, st.min_spp, st.step_spp)
    assert st.samples_uniform == W * H * spp
    assert st.samples_traced == 64 * tile_spp.size * spp


@pytest.mark.parametrize("min_spp,step_spp", [(20, 4), (16, 4)])
def test_threshold_zero_across_buffer_batches(rt, renderer, min_spp, step_spp):
    """A 1 MiB trace buffer holds 15 of the 45-tile frame's samples (7 when batches overlap): passes
    of 20 and 16 samples take several buffer batches that do not end on the 2-sample chunk's
    boundaries, and the carried sums still give rt_render's bits."""
    scene, W, H, spp = 7, 72, 40, 20
    cam, bg = _setup(rt, renderer, scene, W, H)
    full = renderer.render(cam, _params(rt, bg, W, H, spp))
    renderer.set_option(rt.RT_OPT_TRACE_BUF_BYTES, 1 << 20)
    try:
        mean, tile_spp, _, _ = renderer.render_adaptive(cam, _params(rt, bg, W, H, spp), min_spp, step_spp, 0.0)
        st, ast = renderer.stats(), renderer.adaptive_stats()
    finally:
        renderer.set_option(rt.RT_OPT_TRACE_BUF_BYTES, 0)
    fit = (1 << 20) // (45 * 64 * 24)
    assert fit % 2 == 1 and (fit // 2) % 2 == 1       # either batch size is off the chunk grid
    assert ast.spp_chunk == 2 and ast.max_pass_batches > 1
    assert st.n_batches >= ast.passes - 1 + ast.max_pass_batches   # rt_stats counts the call's trace launches
    assert np.array_equal(mean, full) and (tile_spp == spp).all()


def test_threshold_inf_stops_at_min_spp(rt, renderer):
    """+inf stops every tile after the first pass: rt_render's frame at the rounded min_spp."""
    scene, W, H, spp, chunk = 0, 37, 21, 40, 4
    cam, bg = _setup(rt, renderer, scene, W, H)
    mean, tile_spp, _, _ = renderer.render_adaptive(cam, _params(rt, bg, W, H, spp, chunk), 6, 8, float("inf"))
    st = renderer.adaptive_stats()
    assert st.min_spp == 8 and st.passes == 1 and (tile_spp == 8).all()
    assert np.array_equal(mean, renderer.render(cam, _params(rt, bg, W, H, 8, chunk)))


@pytest.mark.parametrize("scene,W,H,threshold", [(0, 40, 24, 0.029), (0, 36, 20, 0.030), (4, 40, 24, 0.030)])
def test_adaptive_counts_and_pixels(rt, renderer, scene, W, H, threshold):
    """spp 96, min 16, step 16, chunk 16. The expected stop counts come from the oracle-derived
    samples and the numpy criterion; the thresholds keep every tested reference E_t at least 0.5 %
    (5000 x the tolerance) away, so the library must reproduce the map exactly. The random scene
    stops at three or more distinct counts; the light scene has only black tiles (min_spp) and lit
    ones (spp). Edge tiles (36x20):
    E_t averages their in-image pixels only, and samples_traced counts all 64 pixel slots of every
    tile, the ones past the image included, because a tile shard traces them."""
    spp, min_spp, step_spp, chunk = 96, 16, 16, 16
    samples = ar.oracle_samples(scene, W, H, spp)
    exp_spp, S, Q, exp_E, exp_se, tested = ar.simulate(samples, W, H, spp, min_spp, step_spp, threshold)
    margin = np.min(np.abs(tested / threshold - 1.0))
    counts = sorted(set(exp_spp.reshape(-1).tolist()))
    print(f"reference: counts {counts}, margin {margin:.4f}")
    assert margin >= 0.005
    if scene == 0:
        assert len(counts) >= 3
    assert min_spp in counts and spp in counts

    cam, bg = _setup(rt, renderer, scene, W, H)
    mean, tile_spp, tile_error, se = renderer.render_adaptive(cam, _params(rt, bg, W, H, spp, chunk), min_spp,
                                                               step_spp, threshold)
    assert np.array_equal(tile_spp, exp_spp)
    n_px = ar.tile_map(exp_spp, W, H)
    for n in counts:
        sel = n_px == n
        uniform = renderer.render(cam, _params(rt, bg, W, H, n, chunk))
        assert np.array_equal(mean[sel], uniform[sel]), n
        ref = ob.render(scene, W, H, n, spp_chunk=chunk)
        d = np.abs(mean[sel] - ref[sel])
        print(f"n = {n}: {int(sel.sum())} pixels, L_inf vs oracle {d.max():.3e}")
        assert d.max() <= LINF and np.all(d <= REL * np.abs(ref[sel])), n
    print(f"max |E_t - ref| {np.abs(tile_error - exp_E).max():.3e}, max |se - ref| {np.abs(se - exp_se).max():.3e}")
    assert ar.close(tile_error, exp_E)
    assert ar.close(se, exp_se)
    st = renderer.adaptive_stats()
    assert st.samples_traced == 64 * int(exp_spp.sum())
    in_image = int(n_px.sum())
    assert (st.samples_traced == in_image) if (W % 8 == 0 and H % 8 == 0) else (st.samples_traced > in_image)
    assert st.samples_uniform == W * H * spp and st.passes == spp // step_spp
    assert st.trace_ms > 0 and st.moments_ms > 0 and st.classify_ms > 0


def test_context_state_is_untouched_and_call_is_deterministic(rt, renderer):
    """The call's private tile order and forced schedule leave the context as it was: a tile order
    set before still deals the same shard, a plain rt_render gives its usual bits, and a second
    call repeats the first."""
    scene, W, H, spp, chunk = 0, 40, 24, 48, 16
    cam, bg = _setup(rt, renderer, scene, W, H)
    full = renderer.render(cam, _params(rt, bg, W, H, spp, chunk))
    order = np.random.default_rng(3).permutation(15)
    shard = dict(row_begin=1, row_stride=3, tile_shard=1)
    raster = renderer.render(cam, _params(rt, bg, W, H, spp, chunk, **shard))
    renderer.set_tile_order(order)
    renderer.set_schedule(rt.RT_SCHED_ITEMS)
    try:
        before = renderer.render(cam, _params(rt, bg, W, H, spp, chunk, **shard))
        a = renderer.render_adaptive(cam, _params(rt, bg, W, H, spp, chunk), 16, 16, 0.04)
        assert renderer.stats().schedule == rt.RT_SCHED_POOL
        after = renderer.render(cam, _params(rt, bg, W, H, spp, chunk, **shard))
        assert renderer.stats().schedule == rt.RT_SCHED_ITEMS
        b = renderer.render_adaptive(cam, _params(rt, bg, W, H, spp, chunk), 16, 16, 0.04)
        assert np.array_equal(renderer.render(cam, _params(rt, bg, W, H, spp, chunk)), full)
    finally:
        renderer.set_tile_order(None)
        renderer.set_schedule(rt.RT_SCHED_AUTO)
    assert np.array_equal(before, after) and not np.array_equal(before, raster)
    assert len(set(a[1].reshape(-1).tolist())) > 1    # the threshold did split the tiles
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(renderer.render(cam, _params(rt, bg, W, H, spp, chunk)), full)


def test_adaptive_errors(rt, renderer):
    W, H = 32, 24
    cam, bg = _setup(rt, renderer, 0, W, H)
    ok = lambda **kw: _params(rt, bg, W, H, 16, 4, **kw)   # noqa: E731
    renderer.render_adaptive(cam, ok(), 4, 4, 0.05)
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
        renderer.render_adaptive(cam, ok(), 1, 4, 0.05)                     # min_spp < 2
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
        renderer.render_adaptive(cam, ok(), 4, 0, 0.05)                     # step_spp < 1
    for shard in (dict(row_begin=1), dict(row_stride=2), dict(tile_shard=1), dict(row_block=8)):
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
            renderer.render_adaptive(cam, ok(**shard), 4, 4, 0.05)
    renderer.set_precision(rt.RT_PREC_F32)
    try:
        with pytest.raises(rt.RTError, match="RT_ERR_UNSUPPORTED"):
            renderer.render_adaptive(cam, ok(), 4, 4, 0.05)
    finally:
        renderer.set_precision(rt.RT_PREC_F64)
    fresh = rt.Renderer(0)
    try:
        with pytest.raises(rt.RTError, match="RT_ERR_NO_SCENE"):
            fresh.render_adaptive(cam, ok(), 4, 4, 0.05)
    finally:
        fresh.close()
    renderer.render_adaptive(cam, ok(), 4, 4, 0.05)                         # and the context still renders
