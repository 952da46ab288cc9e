"""rt_render_adaptive_halves: rt_render_adaptive plus the means of every pixel's even and of its odd
samples (include/rt/rt_abi.h).

The first four outputs are held to rt_render_adaptive's bit for bit; the halves to the CPU oracle's
per-sample radiances split by parity (tests/adaptive_reference.py), to rt_render at spp 1, and to the
whole sum they add up to; and their bits may depend neither on buffer batches nor on whether the
outputs are host or device memory.
"""
import ctypes

import numpy as np
import pytest

from tests import adaptive_reference as ar

pytestmark = pytest.mark.gpu


def _setup(rt, renderer, scene, W, H):
    renderer.upload(rt.World(1).build_scene(scene))
    return rt.scene_camera(scene, W, H)


def _params(rt, bg, W, H, spp, chunk=0, **kw):
    return rt.Renderer.params(W, H, spp, 50, bg, 1, spp_chunk=chunk, out_format=rt.RT_OUT_F64, **kw)


def _sum_check(mean, tile_spp, mean_a, mean_b, W, H):
    """mean_a n_a + mean_b n_b against mean n: within 1e-12 relative (each side a handful of f64
    roundings of the same samples, added in two orders)."""
    n = ar.tile_map(tile_spp, W, H).astype(np.float64)[..., None]
    na, nb = np.floor((n + 1) / 2), np.floor(n / 2)
    whole, parts = mean * n, mean_a * na + mean_b * nb
    err = np.abs(parts - whole) / np.maximum(np.abs(whole), 1e-300)   # (a black pixel: 0 on both sides)
    print(f"max |mean_a n_a + mean_b n_b - mean n| / |mean n| = {err.max():.3e}")
    assert err.max() <= 1e-12


@pytest.mark.parametrize("threshold", [0.0, 0.03])
@pytest.mark.parametrize("scene,W,H,spp,chunk,min_spp,step_spp",
                         [(0, 37, 21, 40, 4, 8, 8), (5, 32, 32, 17, 0, 4, 6), (7, 72, 40, 20, 0, 6, 3),
                          (7, 72, 40, 20, 3, 6, 3)])
def test_same_bits_as_rt_render_adaptive(rt, renderer, scene, W, H, spp, chunk, min_spp, step_spp, threshold):
    """mean, tile_spp, tile_error and stderr_map with the threshold at 0 and with it on; an odd n
    (17: n_a = 9, n_b = 8), the auto chunk 2 and an odd chunk (3)."""
    cam, bg = _setup(rt, renderer, scene, W, H)
    plain = renderer.render_adaptive(cam, _params(rt, bg, W, H, spp, chunk), min_spp, step_spp, threshold)
    st_plain = renderer.adaptive_stats()
    got = renderer.render_adaptive_halves(cam, _params(rt, bg, W, H, spp, chunk), min_spp, step_spp, threshold)
    st = renderer.adaptive_stats()
    for a, b in zip(plain, got[:4]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    for f in ("passes", "min_spp", "step_spp", "spp_chunk", "tiles", "max_pass_batches", "samples_traced",
              "samples_uniform"):
        assert getattr(st, f) == getattr(st_plain, f), f
    if threshold == 0.0:
        assert (got[1] == spp).all()
    mean_a, mean_b = got[4], got[5]
    assert np.isfinite(mean_a).all() and np.isfinite(mean_b).all() and not np.array_equal(mean_a, mean_b)
    _sum_check(got[0], got[1], mean_a, mean_b, W, H)
    again = renderer.render_adaptive_halves(cam, _params(rt, bg, W, H, spp, chunk), min_spp, step_spp, threshold)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()              # repeats bit for bit


@pytest.mark.parametrize("scene,W,H,threshold", [(0, 40, 24, 0.029), (0, 36, 20, 0.030)])
def test_halves_against_the_oracle(rt, renderer, scene, W, H, threshold):
    """spp 96, min 16, step 16, chunk 16 (test_adaptive_counts_and_pixels' set-up: three or more stop
    counts). Per stop count n, the pixels of those tiles against the oracle-derived samples [:n] split
    by parity: 1e-12 + 1e-9 |ref| (the derived samples carry <= 4e-15)."""
    spp, min_spp, step_spp, chunk = 96, 16, 16, 16
    samples = ar.oracle_samples(scene, W, H, spp)
    cam, bg = _setup(rt, renderer, scene, W, H)
    mean, tile_spp, _, _, mean_a, mean_b = renderer.render_adaptive_halves(cam, _params(rt, bg, W, H, spp, chunk),
                                                                          min_spp, step_spp, threshold)
    counts = sorted(set(tile_spp.reshape(-1).tolist()))
    assert len(counts) >= 3
    n_px = ar.tile_map(tile_spp, W, H)
    for n in counts:
        sel = n_px == n
        for what, got, ref in (("mean_a", mean_a, samples[:n][0::2].mean(0)), ("mean_b", mean_b, samples[:n][1::2].mean(0))):
            d = np.abs(got[sel] - ref[sel])
            tol = 1e-12 + 1e-9 * np.abs(ref[sel])
            print(f"n = {n}: {what} over {int(sel.sum())} pixels, max |got - ref| / tol = {(d / tol).max():.3e}")
            assert np.all(d <= tol), (n, what)
    _sum_check(mean, tile_spp, mean_a, mean_b, W, H)


def test_one_sample_per_half_is_rt_render_at_spp_1(rt, renderer):
    """spp 2, min 2, threshold 0: half A is sample 0 alone, rt_render's frame at spp 1 bit for bit."""
    scene, W, H = 0, 37, 21
    cam, bg = _setup(rt, renderer, scene, W, H)
    one = renderer.render(cam, _params(rt, bg, W, H, 1))
    two = renderer.render(cam, _params(rt, bg, W, H, 2))
    mean, tile_spp, _, _, mean_a, mean_b = renderer.render_adaptive_halves(cam, _params(rt, bg, W, H, 2), 2, 2, 0.0)
    assert (tile_spp == 2).all() and mean.tobytes() == two.tobytes()
    assert mean_a.tobytes() == one.tobytes()
    assert not np.array_equal(mean_b, one)
    _sum_check(mean, tile_spp, mean_a, mean_b, W, H)


@pytest.mark.parametrize("min_spp,step_spp", [(20, 4), (16, 4)])
def test_halves_across_buffer_batches(rt, renderer, min_spp, step_spp):
    """test_threshold_zero_across_buffer_batches' set-up: under a 1 MiB trace buffer the passes take
    several batches that end off the 2-sample chunk's grid (an odd number of samples each, so a
    batch's first sample is odd as often as even); the halves have the one-batch bits."""
    scene, W, H, spp = 7, 72, 40, 20
    cam, bg = _setup(rt, renderer, scene, W, H)
    want = renderer.render_adaptive_halves(cam, _params(rt, bg, W, H, spp), min_spp, step_spp, 0.0)
    assert renderer.adaptive_stats().max_pass_batches == 1
    renderer.set_option(rt.RT_OPT_TRACE_BUF_BYTES, 1 << 20)
    try:
        got = renderer.render_adaptive_halves(cam, _params(rt, bg, W, H, spp), min_spp, step_spp, 0.0)
        ast = renderer.adaptive_stats()
    finally:
        renderer.set_option(rt.RT_OPT_TRACE_BUF_BYTES, 0)
    assert ast.spp_chunk == 2 and ast.max_pass_batches > 1
    for a, b in zip(want, got):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("fmt", ["f64", "f32"])
def test_device_pointers_give_the_host_pointer_bits(rt, renderer, fmt):
    import torch
    scene, W, H, spp, chunk, min_spp, step_spp, threshold = 0, 37, 21, 40, 4, 8, 8, 0.03
    out_format, tdt = (rt.RT_OUT_F64, torch.float64) if fmt == "f64" else (rt.RT_OUT_F32, torch.float32)
    cam, bg = _setup(rt, renderer, scene, W, H)
    p = rt.Renderer.params(W, H, spp, 50, bg, 1, spp_chunk=chunk, out_format=out_format)
    mean, tile_spp, tile_error, se, mean_a, mean_b = renderer.render_adaptive_halves(cam, p, min_spp, step_spp, threshold)
    assert mean_a.dtype == (np.float64 if fmt == "f64" else np.float32)
    dev = {k: torch.full((H, W, 3), 7.0, dtype=tdt, device="cuda:0") for k in ("mean", "a", "b")}
    se_d = torch.zeros((H, W), dtype=torch.float64, device="cuda:0")
    spp_d = torch.zeros(tile_spp.shape, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    renderer.render_adaptive_halves_device(cam, p, min_spp, step_spp, threshold, dev["mean"].data_ptr(),
                                           dev["a"].data_ptr(), dev["b"].data_ptr(), stderr_ptr=se_d.data_ptr(),
                                           tile_spp_ptr=spp_d.data_ptr(), stream=stream.cuda_stream)
    torch.cuda.synchronize()
    assert dev["mean"].cpu().numpy().tobytes() == mean.tobytes()
    assert dev["a"].cpu().numpy().tobytes() == mean_a.tobytes()
    assert dev["b"].cpu().numpy().tobytes() == mean_b.tobytes()
    assert se_d.cpu().numpy().tobytes() == se.tobytes()
    assert np.array_equal(spp_d.cpu().numpy().astype(np.uint32), tile_spp)


def test_halves_errors(rt, renderer):
    W, H = 32, 24
    cam, bg = _setup(rt, renderer, 0, W, H)
    ok = lambda **kw: _params(rt, bg, W, H, 16, 4, **kw)   # noqa: E731
    renderer.render_adaptive_halves(cam, ok(), 4, 4, 0.05)
    lib = rt.load_library()
    mean, a, b = (np.empty((H, W, 3)) for _ in range(3))
    ap = rt.AdaptiveParams(4, 4, 0.05)
    out = rt.AdaptiveOut(mean.ctypes.data, None, None, None)

    def raw(hv):
        p = ok()
        return lib.rt_render_adaptive_halves(renderer.h, ctypes.byref(cam), ctypes.byref(p), ctypes.byref(ap),
                                             ctypes.byref(out), ctypes.byref(hv) if hv is not None else None)

    assert raw(rt.AdaptiveHalves(a.ctypes.data, b.ctypes.data)) == rt.RT_OK
    for hv in (None, rt.AdaptiveHalves(None, b.ctypes.data), rt.AdaptiveHalves(a.ctypes.data, None),
               rt.AdaptiveHalves(a.ctypes.data, a.ctypes.data), rt.AdaptiveHalves(mean.ctypes.data, b.ctypes.data)):
        assert rt.ERRORS.get(raw(hv)) == "RT_ERR_INVALID"
        assert lib.rt_last_error()
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
        renderer.render_adaptive_halves(cam, ok(), 1, 4, 0.05)              # rt_render_adaptive's own errors
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
        renderer.render_adaptive_halves(cam, ok(tile_shard=1), 4, 4, 0.05)
    renderer.set_precision(rt.RT_PREC_F32)
    try:
        with pytest.raises(rt.RTError, match="RT_ERR_UNSUPPORTED"):
            renderer.render_adaptive_halves(cam, ok(), 4, 4, 0.05)
    finally:
        renderer.set_precision(rt.RT_PREC_F64)
    fresh = rt.Renderer(0)
    try:
        with pytest.raises(rt.RTError, match="RT_ERR_NO_SCENE"):
            fresh.render_adaptive_halves(cam, ok(), 4, 4, 0.05)
    finally:
        fresh.close()
    again = renderer.render_adaptive_halves(cam, ok(), 4, 4, 0.05)          # and the context still renders
    assert again[0].tobytes() == renderer.render_adaptive(cam, ok(), 4, 4, 0.05)[0].tobytes()
