"""rt_denoise_atrous on the device: the variance-guided a-trous wavelet filter of
include/rt/rt_abi.h.

Every case filters the library's own rt_render_adaptive frame with the library's own
rt_render_features buffers at 8 spp as guides, as tests/test_gpu_denoise_guided.py sets them up; the
numpy restatement of tests/denoise_atrous_reference.py and rt_denoise_atrous_host run on the same
arrays. Tolerances: tests/denoise_reference.py's (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded
reference in f32). The frames are tests/test_gpu_denoise.py's, and one 72 x 9 frame in which a
step-32 tap (level 6) lands inside the image.
"""
import numpy as np
import pytest

from tests import denoise_atrous_reference as atr
from tests import denoise_guided_reference as gr
from tests import denoise_reference as dr

pytestmark = pytest.mark.gpu

#         scene, W, H, spp, chunk, min, step, threshold
RENDERS = {"random_counts": (0, 40, 24, 96, 16, 16, 16, 0.029),
           "cornell": (5, 40, 40, 16, 0, 8, 8, 0.0),
           "random_ragged": (0, 37, 21, 16, 0, 8, 8, 0.0),
           "random_tiny": (0, 9, 5, 16, 0, 8, 8, 0.0),
           "random_wide": (0, 72, 9, 16, 0, 8, 8, 0.0)}
FEATURE_SPP = 8
SIGMAS = (0.1, 0.2, 0.1)
SIGMA_L = atr.SIGMA_L
LEVELS = [1, 2, 3, 5, 6]
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
    """(mean f64, se, albedo, normal, depth) of one adaptive render and one feature pass, rendered once."""
    if name not in _frames:
        cam, p, pf = _setup(rt, renderer, name)
        _, _, _, _, _, min_spp, step_spp, threshold = RENDERS[name]
        mean, _, _, se = renderer.render_adaptive(cam, p, min_spp, step_spp, threshold)
        guides = renderer.render_features(cam, pf)
        for a in (mean, se, *guides):
            assert np.isfinite(a).all()
            a.setflags(write=False)
        _frames[name] = (mean, se, *guides)
    return _frames[name]


def _scratch(levels, W, H):
    return (0 if levels == 1 else 1 if levels == 2 else 2) * 32 * W * H


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("name", list(RENDERS))
def test_device_matches_numpy_and_host(rt, renderer, name, levels):
    mean, se, *guides = _frame(rt, renderer, name)
    H, W = se.shape
    outs = {}
    for dtype in (np.float64, np.float32):
        m = mean.astype(dtype)
        for variant in atr.VARIANTS:
            a, n, z, dem = atr.variant_args(variant, guides)
            got, got_se = renderer.denoise_atrous(m, se, a, n, z, SIGMAS, levels, SIGMA_L, dem)
            st = renderer.atrous_stats()
            what = f"{name} {np.dtype(dtype).name} L={levels} {variant}"
            assert got.dtype == m.dtype and got.shape == m.shape and got_se.dtype == np.float64 and got_se.shape == se.shape
            ref, ref_se = atr.atrous(m, se, levels, SIGMA_L, a, n, z, SIGMAS, dem)
            dr.check(got, ref, what + " out vs numpy")
            dr.check(got_se, ref_se, what + " stderr_out vs numpy")
            host, host_se = rt.denoise_atrous_host(m, se, a, n, z, SIGMAS, levels, SIGMA_L, dem)
            dr.check(got, host, what + " out vs the host filter")
            dr.check(got_se, host_se, what + " stderr_out vs the host filter")
            again, again_se = renderer.denoise_atrous(m, se, a, n, z, SIGMAS, levels, SIGMA_L, dem)
            assert np.array_equal(again, got) and np.array_equal(again_se, got_se)      # repeats bit for bit
            assert st.kernel_ms > 0 and st.levels == levels and st.scratch_bytes == _scratch(levels, W, H)
            no_se, none = renderer.denoise_atrous(m, se, a, n, z, SIGMAS, levels, SIGMA_L, dem, want_stderr=False)
            assert none is None and np.array_equal(no_se, got)
            outs[dtype, variant] = got
            print(f"{what}: kernel {st.kernel_ms:.3f} ms, scratch {st.scratch_bytes} B")
        if W > 1 and H > 1:
            assert not np.array_equal(outs[dtype, "guided"], outs[dtype, "unguided"])       # the guides act
            assert not np.array_equal(outs[dtype, "guided"], outs[dtype, "demodulated"])


@pytest.mark.parametrize("name,fmt", [("random_counts", "f64"), ("random_ragged", "f32")])
def test_device_pointer_chain_is_the_host_pointer_chain(rt, renderer, name, fmt):
    """rt_render_adaptive, rt_render_features and rt_denoise_atrous into torch tensors on one torch
    stream, no host round trip, against the same three calls on host arrays: the same bits."""
    import torch
    _, W, H, _, _, min_spp, step_spp, threshold = RENDERS[name]
    out_format, tdt = (rt.RT_OUT_F64, torch.float64) if fmt == "f64" else (rt.RT_OUT_F32, torch.float32)
    cam, p, pf = _setup(rt, renderer, name, out_format)
    mean_h, _, _, se_h = renderer.render_adaptive(cam, p, min_spp, step_spp, threshold)
    guides_h = renderer.render_features(cam, pf)
    want, want_se = renderer.denoise_atrous(mean_h, se_h, *guides_h, SIGMAS, 5, SIGMA_L, True)

    f64 = dict(dtype=torch.float64, device="cuda:0")
    mean_d = torch.zeros((H, W, 3), dtype=tdt, device="cuda:0")
    se_d, z_d = torch.zeros((H, W), **f64), torch.zeros((H, W), **f64)
    a_d, n_d = torch.zeros((H, W, 3), **f64), torch.zeros((H, W, 3), **f64)
    out_d = torch.full((H, W, 3), 7.0, dtype=tdt, device="cuda:0")
    se_out_d = torch.full((H, W), 7.0, **f64)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    s = stream.cuda_stream
    renderer.render_adaptive_device(cam, p, min_spp, step_spp, threshold, mean_d.data_ptr(), se_d.data_ptr(), stream=s)
    renderer.render_features_device(cam, pf, a_d.data_ptr(), n_d.data_ptr(), z_d.data_ptr(), stream=s)
    renderer.denoise_atrous_device(mean_d.data_ptr(), se_d.data_ptr(), out_d.data_ptr(), W, H, a_d.data_ptr(),
                                   n_d.data_ptr(), z_d.data_ptr(), SIGMAS, out_format, 5, SIGMA_L, True,
                                   se_out_d.data_ptr(), stream=s)
    assert renderer.atrous_stats().kernel_ms > 0          # waits for the kernels
    torch.cuda.synchronize()
    assert np.array_equal(out_d.cpu().numpy(), want)
    assert np.array_equal(se_out_d.cpu().numpy(), want_se)


def test_scratch_grows_with_work_in_flight(rt, renderer):
    """On a context of its own (no scratch yet): frames of size A, the larger B, then A again, enqueued
    back to back on one torch stream with one synchronisation at the end; each equals its
    host-pointer result. The second call grows the scratch while the first may still run."""
    import torch
    frames = [_frame(rt, renderer, n) for n in ("random_ragged", "cornell", "random_ragged")]
    own = rt.Renderer(0)
    try:
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        dev = []
        for mean, se, a, n, z in frames:
            t = [torch.from_numpy(np.array(x)).to("cuda:0") for x in (mean, se, a, n, z)]
            t += [torch.full(mean.shape, 7.0, dtype=torch.float64, device="cuda:0"),
                  torch.full(se.shape, 7.0, dtype=torch.float64, device="cuda:0")]
            dev.append(t)
        torch.cuda.synchronize()
        for (mean, se, *_), (m_d, se_d, a_d, n_d, z_d, out_d, so_d) in zip(frames, dev):
            H, W = se.shape
            own.denoise_atrous_device(m_d.data_ptr(), se_d.data_ptr(), out_d.data_ptr(), W, H, a_d.data_ptr(),
                                      n_d.data_ptr(), z_d.data_ptr(), SIGMAS, rt.RT_OUT_F64, 5, SIGMA_L, False,
                                      so_d.data_ptr(), stream=stream.cuda_stream)
        torch.cuda.synchronize()
        assert own.atrous_stats().scratch_bytes == _scratch(5, 37, 21)
        for i, ((mean, se, a, n, z), t) in enumerate(zip(frames, dev)):
            want, want_se = own.denoise_atrous(mean, se, a, n, z, SIGMAS, 5, SIGMA_L, False)
            assert np.array_equal(t[5].cpu().numpy(), want), i
            assert np.array_equal(t[6].cpu().numpy(), want_se), i
    finally:
        own.close()


@pytest.mark.parametrize("variant", atr.VARIANTS)
def test_non_finite_pixels_behave_as_on_the_host(rt, renderer, variant):
    mean, se, *guides = (np.array(x) for x in _frame(rt, renderer, "random_ragged"))
    mean[7, 11, 1] = np.nan
    se[15, 30] = np.inf
    if variant == "demodulated":
        guides[0][3, 4, 2] = np.nan
    a, n, z, dem = atr.variant_args(variant, guides)
    for levels in (1, 3, 6):
        got, got_se = renderer.denoise_atrous(mean, se, a, n, z, SIGMAS, levels, SIGMA_L, dem)
        host, host_se = rt.denoise_atrous_host(mean, se, a, n, z, SIGMAS, levels, SIGMA_L, dem)
        ref, ref_se = atr.atrous(mean, se, levels, SIGMA_L, a, n, z, SIGMAS, dem)
        for x, y, what in ((got, host, "out vs host"), (got_se, host_se, "stderr_out vs host"),
                           (got, ref, "out vs numpy"), (got_se, ref_se, "stderr_out vs numpy")):
            dr.check(x, y, f"non-finite {variant} L={levels} {what}")
        assert got[7, 11].tobytes() == mean[7, 11].tobytes() and got[15, 30].tobytes() == mean[15, 30].tobytes()
        assert np.isnan(got).sum() == 1 and np.isinf(got_se[15, 30]) and np.isfinite(got[3, 4]).all()


def test_invalid_arguments_leave_the_context_usable(rt, renderer):
    mean, se, a, n, z = _frame(rt, renderer, "random_tiny")
    want = renderer.denoise_atrous(mean, se, a, n, z, SIGMAS, 3, SIGMA_L, True)

    def still_filters():
        got = renderer.denoise_atrous(mean, se, a, n, z, SIGMAS, 3, SIGMA_L, True)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])

    bad = [dict(levels=0), dict(levels=7), dict(sigma_l=0.0), dict(sigma_l=float("nan")), dict(sigma_l=float("inf")),
           dict(sigmas=(0.0, 0.2, 0.1)), dict(sigmas=(0.1, float("nan"), 0.1)), dict(sigmas=(0.1, 0.2, float("inf")))]
    for kw in bad:
        args = dict(sigmas=SIGMAS, levels=3, sigma_l=SIGMA_L, demodulate=True)
        args.update(kw)
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
            renderer.denoise_atrous(mean, se, a, n, z, **args)
        still_filters()
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):           # demodulate without albedo
        renderer.denoise_atrous(mean, se, None, n, z, SIGMAS, 3, SIGMA_L, True)
    still_filters()
    import ctypes
    m, s = np.ascontiguousarray(mean), np.ascontiguousarray(se)
    p = rt.AtrousParams(9, 5, rt.RT_OUT_F64, 0, 3, 0, SIGMA_L, None)
    out, se_out = np.empty_like(m), np.empty_like(s)
    lib = rt.load_library()
    for o, so in ((m, se_out), (out, s)):                             # out == mean, stderr_out == stderr_map
        rc = lib.rt_denoise_atrous(renderer.h, ctypes.byref(p), m.ctypes.data, s.ctypes.data, None, o.ctypes.data,
                                   so.ctypes.data)
        assert rt.ERRORS.get(rc) == "RT_ERR_INVALID"
        still_filters()
    p.demodulate = 2
    assert rt.ERRORS.get(lib.rt_denoise_atrous(renderer.h, ctypes.byref(p), m.ctypes.data, s.ctypes.data, None,
                                               out.ctypes.data, se_out.ctypes.data)) == "RT_ERR_INVALID"
    still_filters()


def test_the_other_filters_keep_their_bits(rt, renderer):
    """rt_denoise and rt_denoise_guided on the same context before and after a-trous calls (which
    allocate and grow the context's scratch): the same bits, and the numpy references' values."""
    mean, se, a, n, z = _frame(rt, renderer, "random_ragged")
    plain = renderer.denoise(mean, se, 5, 2, 1.0)
    guided = renderer.denoise_guided(mean, se, a, n, z, SIGMAS, 5, 2, 1.0)
    for levels in (2, 6):
        renderer.denoise_atrous(mean, se, a, n, z, SIGMAS, levels, SIGMA_L, True)
        assert np.array_equal(renderer.denoise(mean, se, 5, 2, 1.0), plain)
        assert np.array_equal(renderer.denoise_guided(mean, se, a, n, z, SIGMAS, 5, 2, 1.0), guided)
    dr.check(plain, dr.denoise(mean, se, 5, 2, 1.0), "rt_denoise after a-trous")
    dr.check(guided, gr.denoise_guided(mean, se, 5, 2, 1.0, a, n, z, SIGMAS), "rt_denoise_guided after a-trous")
