"""rt_denoise_cross on the device: NL-means over two half frames, each filtered with the other's
weights, and the error map read off their difference (include/rt/rt_abi.h).

Every case filters the library's own rt_render_adaptive_halves outputs
(tests/test_gpu_adaptive_halves.py holds those to their references), with and without the library's
own rt_render_features buffers at 8 spp as guides; the numpy restatement of
tests/denoise_cross_reference.py and rt_denoise_cross_host run on the same arrays. Tolerances:
tests/denoise_reference.py's (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded reference in f32),
for out and for stderr_out. The frames are tests/test_gpu_denoise.py's: three or more distinct tile
counts (40x24), 6.25 filter tiles (40x40), sides that are no multiple of the 16-pixel tile (37x21)
and a frame smaller than any window (9x5).
"""
import ctypes

import numpy as np
import pytest

from tests import denoise_cross_reference as cr
from tests import denoise_reference as dr

pytestmark = pytest.mark.gpu

#         scene, W, H, spp, chunk, min, step, threshold   (tests/test_gpu_denoise.py RENDERS)
RENDERS = {"random_counts": (0, 40, 24, 96, 16, 16, 16, 0.029),
           "cornell": (5, 40, 40, 16, 0, 8, 8, 0.0),
           "random_ragged": (0, 37, 21, 16, 0, 8, 8, 0.0),
           "random_tiny": (0, 9, 5, 16, 0, 8, 8, 0.0)}
FEATURE_SPP = 8
SIGMAS = (0.1, 0.2, 0.1)
_frames = {}


def _setup(rt, renderer, name, out_format=None):
    scene, W, H, spp, chunk, *_ = RENDERS[name]
    renderer.upload(rt.World(1).build_scene(scene))
    cam, bg = rt.scene_camera(scene, W, H)
    p = rt.Renderer.params(W, H, spp, 50, bg, 1, spp_chunk=chunk,
                           out_format=rt.RT_OUT_F64 if out_format is None else out_format)
    pf = rt.Renderer.params(W, H, FEATURE_SPP, 50, bg, 1, out_format=rt.RT_OUT_F64)
    return cam, p, pf


def _frame(rt, renderer, name):
    """(mean, mean_a, mean_b f64, se, (albedo, normal, depth)) of one adaptive render with halves and
    one feature pass, rendered once."""
    if name not in _frames:
        cam, p, pf = _setup(rt, renderer, name)
        _, _, _, _, _, min_spp, step_spp, threshold = RENDERS[name]
        mean, tile_spp, _, se, a, b = renderer.render_adaptive_halves(cam, p, min_spp, step_spp, threshold)
        if name == "random_counts":
            assert len(set(tile_spp.reshape(-1).tolist())) >= 3
        guides = renderer.render_features(cam, pf)
        for x in (mean, a, b, se, *guides):
            assert np.isfinite(x).all()
            x.setflags(write=False)
        assert se.max() > 0 and not np.array_equal(a, b)
        _frames[name] = (mean, a, b, se, guides)
    return _frames[name]


def _lds(radius, patch):
    sw, pw, ps = 16 + 2 * (radius + patch), 16 + 2 * patch, 16 if patch == 0 else 48
    return (3 * sw * sw + 4 * pw * ps) * 8


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
@pytest.mark.parametrize("name", list(RENDERS))
def test_device_filter_matches_numpy_and_host(rt, renderer, name, radius, patch, k, guided):
    _, a64, b64, se, guides = _frame(rt, renderer, name)
    g = dict(albedo=guides[0], normal=guides[1], depth=guides[2], sigmas=SIGMAS) if guided else {}
    for dtype in (np.float64, np.float32):
        a, b = a64.astype(dtype), b64.astype(dtype)
        kw = dict(radius=radius, patch=patch, k=k, variance_scale=cr.SCALE, **g)
        got, got_se = renderer.denoise_cross(a, b, se, **kw)
        st = renderer.cross_stats()
        what = f"{name} {np.dtype(dtype).name} r={radius} f={patch} k={k} guided={guided}"
        assert got.dtype == a.dtype and got.shape == a.shape and got_se.shape == se.shape
        ref, ref_se = cr.denoise_cross(a, b, se, radius, patch, k, cr.SCALE, **g)
        host, host_se = rt.denoise_cross_host(a, b, se, **kw)
        dr.check(got, ref, what + " vs numpy")
        dr.check(got_se, ref_se, what + " stderr_out vs numpy")
        dr.check(got, host, what + " vs the host filter")
        dr.check(got_se, host_se, what + " stderr_out vs the host filter")
        again, again_se = renderer.denoise_cross(a, b, se, **kw)                  # repeats bit for bit
        assert again.tobytes() == got.tobytes() and again_se.tobytes() == got_se.tobytes()
        assert st.kernel_ms > 0 and (st.radius, st.patch) == (radius, patch)
        assert st.lds_bytes == _lds(radius, patch) and st.scratch_bytes == 8 * se.size
        only, none = renderer.denoise_cross(a, b, se, want_stderr=False, **kw)   # one launch, no scratch
        assert none is None and only.tobytes() == got.tobytes() and renderer.cross_stats().scratch_bytes == 0
        print(f"{what}: kernels {st.kernel_ms:.3f} ms, LDS {st.lds_bytes} B")
    assert _lds(10, 3) == 76128


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
@pytest.mark.parametrize("name", ["random_counts", "random_ragged", "random_tiny"])
def test_same_halves_are_the_existing_kernels(rt, renderer, name, radius, patch, k, guided):
    """mean_a = mean_b = M at scale 1 against renderer.denoise / denoise_guided. Observed on an
    MI355X: identical bits in every case (0 ulp in f32, 0.0 in f64), so the shared arithmetic
    compiles alike in both kernels, and identical bits are what is asserted (after the device-host
    exp bound, which prints the distance); the error map is 0."""
    mean, _, _, se, guides = _frame(rt, renderer, name)
    g = dict(albedo=guides[0], normal=guides[1], depth=guides[2], sigmas=SIGMAS) if guided else {}
    for dtype in (np.float64, np.float32):
        m = mean.astype(dtype)
        got, got_se = renderer.denoise_cross(m, m, se, radius=radius, patch=patch, k=k, variance_scale=1.0, **g)
        plain = renderer.denoise_guided(m, se, *guides, SIGMAS, radius, patch, k) if guided else \
            renderer.denoise(m, se, radius, patch, k)
        dr.check(got, plain, f"{name} r={radius} f={patch} same halves vs the plain kernel")   # within the exp bound
        assert got.tobytes() == plain.tobytes()
        assert np.array_equal(got_se, np.zeros_like(se))


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("radius,patch,k", dr.PARAMS[:3])
def test_swapping_the_halves_changes_no_bit(rt, renderer, radius, patch, k, guided):
    _, a, b, se, guides = _frame(rt, renderer, "random_ragged")
    g = dict(albedo=guides[0], normal=guides[1], depth=guides[2], sigmas=SIGMAS) if guided else {}
    for dtype in (np.float64, np.float32):
        kw = dict(radius=radius, patch=patch, k=k, variance_scale=cr.SCALE, **g)
        o1, s1 = renderer.denoise_cross(a.astype(dtype), b.astype(dtype), se, **kw)
        o2, s2 = renderer.denoise_cross(b.astype(dtype), a.astype(dtype), se, **kw)
        assert o1.tobytes() == o2.tobytes() and s1.tobytes() == s2.tobytes()


@pytest.mark.parametrize("radius,patch,k", dr.PARAMS[:3])
def test_bad_pixels_behave_as_on_the_host(rt, renderer, radius, patch, k):
    _, a, b, se, _ = (np.array(x) if isinstance(x, np.ndarray) else x for x in _frame(rt, renderer, "random_ragged"))
    a[7, 11, 1] = np.nan
    b[15, 30] = np.inf
    se[3, 4], se[18, 20] = np.inf, np.nan
    got, got_se = renderer.denoise_cross(a, b, se, radius=radius, patch=patch, k=k, variance_scale=cr.SCALE)
    ref, ref_se = cr.denoise_cross(a, b, se, radius, patch, k, cr.SCALE)
    rest = np.ones(se.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        for q in ((7, 11), (15, 30), (3, 4), (18, 20)):
            assert np.array_equal(got[q], 0.5 * (a[q] + b[q]), equal_nan=True)
            rest[q] = False
    assert np.isfinite(got[rest]).all()
    dr.check(got[rest], ref[rest], f"bad pixels r={radius} f={patch}")
    dr.check(got_se, ref_se, f"bad pixels r={radius} f={patch} stderr_out")


@pytest.mark.parametrize("name,fmt", [("random_counts", "f64"), ("random_ragged", "f32")])
def test_device_pointer_chain_is_the_host_pointer_chain(rt, renderer, name, fmt):
    """rt_render_adaptive_halves, rt_render_features and rt_denoise_cross into torch tensors on one
    torch stream, no host round trip, against the same three calls on host arrays: the same bits."""
    import torch
    _, W, H, _, _, min_spp, step_spp, threshold = RENDERS[name]
    out_format, tdt = (rt.RT_OUT_F64, torch.float64) if fmt == "f64" else (rt.RT_OUT_F32, torch.float32)
    cam, p, pf = _setup(rt, renderer, name, out_format)
    _, _, _, se_h, a_h, b_h = renderer.render_adaptive_halves(cam, p, min_spp, step_spp, threshold)
    guides_h = renderer.render_features(cam, pf)
    want, want_se = renderer.denoise_cross(a_h, b_h, se_h, *guides_h, SIGMAS, 10, 3, 0.45, cr.SCALE)

    f64 = dict(dtype=torch.float64, device="cuda:0")
    mean_d, ma_d, mb_d = (torch.zeros((H, W, 3), dtype=tdt, device="cuda:0") for _ in range(3))
    se_d, z_d = torch.zeros((H, W), **f64), torch.zeros((H, W), **f64)
    al_d, n_d = torch.zeros((H, W, 3), **f64), torch.zeros((H, W, 3), **f64)
    out_d = torch.full((H, W, 3), 7.0, dtype=tdt, device="cuda:0")
    so_d = torch.full((H, W), 7.0, **f64)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    s = stream.cuda_stream
    renderer.render_adaptive_halves_device(cam, p, min_spp, step_spp, threshold, mean_d.data_ptr(), ma_d.data_ptr(),
                                           mb_d.data_ptr(), stderr_ptr=se_d.data_ptr(), stream=s)
    renderer.render_features_device(cam, pf, al_d.data_ptr(), n_d.data_ptr(), z_d.data_ptr(), stream=s)
    renderer.denoise_cross_device(ma_d.data_ptr(), mb_d.data_ptr(), se_d.data_ptr(), out_d.data_ptr(), W, H,
                                  al_d.data_ptr(), n_d.data_ptr(), z_d.data_ptr(), SIGMAS, out_format, 10, 3, 0.45,
                                  cr.SCALE, stderr_out_ptr=so_d.data_ptr(), stream=s)
    st = renderer.cross_stats()                            # waits for the kernels
    assert st.kernel_ms > 0 and st.scratch_bytes == 8 * W * H
    torch.cuda.synchronize()
    assert ma_d.cpu().numpy().tobytes() == a_h.tobytes() and mb_d.cpu().numpy().tobytes() == b_h.tobytes()
    assert out_d.cpu().numpy().tobytes() == want.tobytes()
    assert so_d.cpu().numpy().tobytes() == want_se.tobytes()


def test_scratch_grows_with_work_in_flight(rt, renderer):
    """On a context of its own (no scratch yet): frames of size A, the larger B, then A again, in f64
    with stderr_out, enqueued back to back on one torch stream with one synchronisation at the end;
    each out and stderr_out equals its host-pointer result bit for bit. The second call grows the e
    scratch while the first may still run."""
    import torch
    frames = [_frame(rt, renderer, n) for n in ("random_ragged", "cornell", "random_ragged")]
    own = rt.Renderer(0)
    try:
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        dev = []
        for _, a, b, se, _ in frames:
            t = [torch.from_numpy(np.array(x)).to("cuda:0") for x in (a, b, se)]
            t += [torch.full(a.shape, 7.0, dtype=torch.float64, device="cuda:0"),
                  torch.full(se.shape, 7.0, dtype=torch.float64, device="cuda:0")]
            dev.append(t)
        torch.cuda.synchronize()
        for a_d, b_d, se_d, out_d, so_d in dev:
            H, W = se_d.shape
            own.denoise_cross_device(a_d.data_ptr(), b_d.data_ptr(), se_d.data_ptr(), out_d.data_ptr(), W, H,
                                     out_format=rt.RT_OUT_F64, radius=10, patch=3, k=0.45, variance_scale=cr.SCALE,
                                     stderr_out_ptr=so_d.data_ptr(), stream=stream.cuda_stream)
        torch.cuda.synchronize()
        assert own.cross_stats().scratch_bytes == 8 * 37 * 21
        for i, ((_, a, b, se, _), t) in enumerate(zip(frames, dev)):
            want, want_se = own.denoise_cross(a, b, se, radius=10, patch=3, k=0.45, variance_scale=cr.SCALE)
            assert t[3].cpu().numpy().tobytes() == want.tobytes(), i
            assert t[4].cpu().numpy().tobytes() == want_se.tobytes(), i
    finally:
        own.close()


def test_fresh_context_without_a_scene(rt, renderer):
    _, a, b, se, _ = _frame(rt, renderer, "random_ragged")
    want, want_se = renderer.denoise_cross(a, b, se, radius=5, patch=2, k=1.0)
    fresh = rt.Renderer(0)
    try:
        got, got_se = fresh.denoise_cross(a, b, se, radius=5, patch=2, k=1.0)
        st = fresh.cross_stats()
        assert st.kernel_ms > 0 and st.lds_bytes == _lds(5, 2) and st.scratch_bytes == 8 * se.size
    finally:
        fresh.close()
    assert got.tobytes() == want.tobytes() and got_se.tobytes() == want_se.tobytes()


def test_invalid_arguments(rt, renderer):
    W, H = 12, 7
    a, b, se = np.ones((H, W, 3)), np.ones((H, W, 3)), np.zeros((H, W))
    out, so = np.empty((H, W, 3)), np.empty((H, W))
    lib = rt.load_library()
    ptr = lambda x: x.ctypes.data if x is not None else None   # noqa: E731
    ok = lambda **kw: rt.CrossParams(**{**dict(width=W, height=H, format=rt.RT_OUT_F64, on_device=0, radius=3,   # noqa: E731
                                               patch=1, k=0.45, variance_scale=2.0, stream=None), **kw})

    def call(h, params, ma, mb, s, g, o, e):
        return lib.rt_denoise_cross(h, ctypes.byref(params) if params is not None else None, ptr(ma), ptr(mb), ptr(s),
                                    ctypes.byref(g) if g is not None else None, ptr(o), ptr(e))

    h = renderer.h
    assert call(h, ok(), a, b, se, None, out, so) == rt.RT_OK
    assert call(h, ok(), a, a, se, None, out, None) == rt.RT_OK
    bad = [(None, ok(), a, b, se, None, out, so), (h, None, a, b, se, None, out, so), (h, ok(), None, b, se, None, out, so),
           (h, ok(), a, None, se, None, out, so), (h, ok(), a, b, None, None, out, so), (h, ok(), a, b, se, None, None, so),
           (h, ok(), a, b, se, None, a, so), (h, ok(), a, b, se, None, b, so), (h, ok(), a, b, se, None, out, se)]
    bad += [(h, ok(**kw), a, b, se, None, out, so) for kw in (
        dict(format=2), dict(format=-1), dict(width=0), dict(height=0), dict(width=-3), dict(radius=0), dict(radius=11),
        dict(patch=-1), dict(patch=4), dict(k=0.0), dict(k=-1.0), dict(k=float("inf")), dict(k=float("nan")),
        dict(variance_scale=0.0), dict(variance_scale=-2.0), dict(variance_scale=float("inf")),
        dict(variance_scale=float("nan")))]
    bad.append((h, ok(), a, b, se, rt.DenoiseGuides(None, None, se.ctypes.data, 1.0, 1.0, 0.0), out, so))
    for args in bad:
        assert rt.ERRORS.get(call(*args)) == "RT_ERR_INVALID", args
        assert lib.rt_last_error()
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
        renderer.denoise_cross(a, b, se, radius=11)
    got, got_se = renderer.denoise_cross(a, b, se, radius=3, patch=1, k=0.45)     # and the context still filters
    assert np.array_equal(got, a) and np.array_equal(got_se, se)
