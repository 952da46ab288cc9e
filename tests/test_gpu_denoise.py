"""rt_denoise on the device: the variance-guided NL-means filter of include/rt/rt_abi.h.

Every case filters the library's own rt_render_adaptive outputs (tests/test_gpu_adaptive.py holds
those to their references); the numpy restatement of tests/denoise_reference.py runs on the same
arrays. Tolerances: that module's (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded reference in
f32). The frames: three or more distinct tile counts (40x24), a frame the size of 6.25 tiles
(40x40), one whose sides are no multiple of the 16-pixel tile (37x21: 2.3 x 1.3 tiles) and one
smaller than any window (9x5).
"""
import ctypes

import numpy as np
import pytest

from tests import denoise_reference as dr

pytestmark = pytest.mark.gpu

#         scene, W, H, spp, chunk, min, step, threshold
RENDERS = {"random_counts": (0, 40, 24, 96, 16, 16, 16, 0.029),
           "cornell": (5, 40, 40, 16, 0, 8, 8, 0.0),
           "random_ragged": (0, 37, 21, 16, 0, 8, 8, 0.0),
           "random_tiny": (0, 9, 5, 16, 0, 8, 8, 0.0)}
_frames = {}
_refs = {}


def _frame(rt, renderer, name):
    """(mean f64, se) of one adaptive render, rendered once."""
    if name not in _frames:
        scene, W, H, spp, chunk, min_spp, step_spp, threshold = RENDERS[name]
        renderer.upload(rt.World(1).build_scene(scene))
        cam, bg = rt.scene_camera(scene, W, H)
        p = rt.Renderer.params(W, H, spp, 50, bg, 1, spp_chunk=chunk, out_format=rt.RT_OUT_F64)
        mean, tile_spp, _, se = renderer.render_adaptive(cam, p, min_spp, step_spp, threshold)
        if name == "random_counts":
            assert len(set(tile_spp.reshape(-1).tolist())) >= 3
        assert np.isfinite(mean).all() and np.isfinite(se).all() and se.max() > 0
        for a in (mean, se):
            a.setflags(write=False)
        _frames[name] = (mean, se)
    return _frames[name]


def _reference(name, mean, se, dtype, radius, patch, k):
    key = (name, np.dtype(dtype).name, radius, patch, k)
    if key not in _refs:
        _refs[key] = dr.denoise(mean.astype(dtype), se, radius, patch, k)
        _refs[key].setflags(write=False)
    return _refs[key]


@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
@pytest.mark.parametrize("name", list(RENDERS))
def test_device_filter_matches_numpy_and_host(rt, renderer, name, radius, patch, k):
    mean, se = _frame(rt, renderer, name)
    for dtype in (np.float64, np.float32):
        m = mean.astype(dtype)
        got = renderer.denoise(m, se, radius, patch, k)
        st = renderer.denoise_stats()
        what = f"{name} {np.dtype(dtype).name} r={radius} f={patch} k={k}"
        assert got.dtype == m.dtype and got.shape == m.shape
        dr.check(got, _reference(name, mean, se, dtype, radius, patch, k), what + " vs numpy")
        dr.check(got, rt.denoise_host(m, se, radius, patch, k), what + " vs rt_denoise_host")
        assert np.array_equal(renderer.denoise(m, se, radius, patch, k), got)      # repeats bit for bit
        assert st.kernel_ms > 0 and 0 < st.lds_bytes <= 65536 and (st.radius, st.patch) == (radius, patch)
        print(f"{what}: kernel {st.kernel_ms:.3f} ms, LDS {st.lds_bytes} B")


@pytest.mark.parametrize("name,fmt", [("random_counts", "f64"), ("random_ragged", "f32"), ("random_tiny", "f64")])
def test_device_pointer_path_is_the_host_pointer_path(rt, renderer, name, fmt):
    """rt_render_adaptive with out_on_device into torch tensors, rt_denoise over them on a torch
    stream with no host round trip, the result read back through the tensor: the host-pointer
    path's bits."""
    import torch
    scene, W, H, spp, chunk, min_spp, step_spp, threshold = RENDERS[name]
    out_format, tdt = (rt.RT_OUT_F64, torch.float64) if fmt == "f64" else (rt.RT_OUT_F32, torch.float32)
    renderer.upload(rt.World(1).build_scene(scene))
    cam, bg = rt.scene_camera(scene, W, H)
    p = rt.Renderer.params(W, H, spp, 50, bg, 1, spp_chunk=chunk, out_format=out_format)
    mean_h, _, _, se_h = renderer.render_adaptive(cam, p, min_spp, step_spp, threshold)
    want = renderer.denoise(mean_h, se_h, 10, 3, 0.45)

    mean_d = torch.zeros((H, W, 3), dtype=tdt, device="cuda:0")
    se_d = torch.zeros((H, W), dtype=torch.float64, device="cuda:0")
    out_d = torch.full((H, W, 3), 7.0, dtype=tdt, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    renderer.render_adaptive_device(cam, p, min_spp, step_spp, threshold, mean_d.data_ptr(), se_d.data_ptr(),
                                    stream=stream.cuda_stream)
    renderer.denoise_device(mean_d.data_ptr(), se_d.data_ptr(), out_d.data_ptr(), W, H, out_format, 10, 3, 0.45,
                            stream=stream.cuda_stream)
    st = renderer.denoise_stats()                     # waits for the kernel
    assert st.kernel_ms > 0
    torch.cuda.synchronize()
    assert np.array_equal(mean_d.cpu().numpy(), mean_h) and np.array_equal(se_d.cpu().numpy(), se_h)
    assert np.array_equal(out_d.cpu().numpy(), want)


def test_fresh_context_without_a_scene(rt, renderer):
    mean, se = _frame(rt, renderer, "random_ragged")
    want = renderer.denoise(mean, se, 5, 2, 1.0)
    fresh = rt.Renderer(0)
    try:
        got = fresh.denoise(mean, se, 5, 2, 1.0)
        assert fresh.denoise_stats().kernel_ms > 0
    finally:
        fresh.close()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
def test_nan_and_inf_stay_where_they_are(rt, renderer, radius, patch, k):
    mean, se = (np.array(a) for a in _frame(rt, renderer, "random_ragged"))
    mean[7, 11] = np.nan
    mean[15, 30, 1] = np.inf
    se[3, 4], se[18, 20] = np.inf, np.nan
    got = renderer.denoise(mean, se, radius, patch, k)
    assert np.isnan(got[7, 11]).all()
    rest = np.ones(mean.shape[:2], dtype=bool)
    for y, x in ((15, 30), (3, 4), (18, 20)):
        assert np.array_equal(got[y, x], mean[y, x])
        rest[y, x] = False
    rest[7, 11] = False
    assert np.isfinite(got[rest]).all()
    dr.check(got[rest], dr.denoise(mean, se, radius, patch, k)[rest], f"NaN / Inf r={radius} f={patch}")


def test_invalid_arguments(rt, renderer):
    W, H = 12, 7
    mean, se, out = np.ones((H, W, 3)), np.zeros((H, W)), np.empty((H, W, 3))
    lib = rt.load_library()
    ptr = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    ok = lambda **kw: rt.DenoiseParams(**{**dict(width=W, height=H, format=rt.RT_OUT_F64, on_device=0, radius=3,   # noqa: E731
                                                 patch=1, k=0.45, stream=None), **kw})

    def call(h, params, m, s, o):
        return lib.rt_denoise(h, ctypes.byref(params) if params is not None else None, ptr(m), ptr(s), ptr(o))

    assert call(renderer.h, ok(), mean, se, out) == rt.RT_OK
    bad = [(None, ok(), mean, se, out), (renderer.h, None, mean, se, out), (renderer.h, ok(), None, se, out),
           (renderer.h, ok(), mean, None, out), (renderer.h, ok(), mean, se, None), (renderer.h, ok(), mean, se, mean)]
    bad += [(renderer.h, ok(**kw), mean, se, out) for kw in (
        dict(format=2), dict(format=-1), dict(width=0), dict(height=0), dict(width=-3), dict(radius=0), dict(radius=11),
        dict(patch=-1), dict(patch=4), dict(k=0.0), dict(k=-1.0), dict(k=float("inf")), dict(k=float("nan")))]
    for args in bad:
        assert rt.ERRORS.get(call(*args)) == "RT_ERR_INVALID", args
        assert lib.rt_last_error()
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
        renderer.denoise(mean, se, radius=11)
    assert np.array_equal(renderer.denoise(mean, se, 3, 1, 0.45), mean)        # and the context still filters
