"""rt_denoise_pyramid on the device: the multi-scale NL-means filter of include/rt/rt_abi.h.

Every case filters the library's own rt_render_adaptive frame with the library's own
rt_render_features buffers at 8 spp as guides: tests/test_gpu_denoise_atrous.py's frames (40 x 24,
40 x 40, 37 x 21, 9 x 5, 72 x 9: odd sizes, levels of one row, several workgroups of the filter),
rendered once and shared with it. The numpy restatement of tests/denoise_pyramid_reference.py and
rt_denoise_pyramid_host run on the same arrays. Tolerances: tests/denoise_reference.py's
(1e-11 + 1e-11 |ref| in f64, one ulp of the rounded reference in f32).
"""
import ctypes

import numpy as np
import pytest

from tests import denoise_pyramid_reference as pr
from tests import denoise_reference as dr
from tests import test_gpu_denoise_atrous as ta

pytestmark = pytest.mark.gpu

RENDERS = ta.RENDERS
SIGMAS = ta.SIGMAS
WINDOW = (5, 2, 1.0)
LEVELS = pr.LEVELS


def _scratch(W, H, levels, f64, guided):
    """rt_pyramid_stats.scratch_bytes as rt_abi.h lists the frames: per level above 0 C (3), s (1),
    the guides (3 + 3 + 1) and D (3) doubles per pixel; D_0; the widened frame when M is f32; one K
    frame of level 1's size."""
    if levels == 1:
        return 0
    w, h = [W], [H]
    for _ in range(levels - 1):
        w.append((w[-1] + 1) // 2)
        h.append((h[-1] + 1) // 2)
    doubles = (3 if f64 else 6) * W * H + 3 * w[1] * h[1]
    doubles += sum((14 if guided else 7) * a * b for a, b in zip(w[1:], h[1:]))
    return 8 * doubles


def _one(rt, renderer, name, levels, window, frames=None):
    mean, se, *guides = ta._frame(rt, renderer, name) if frames is None else frames
    H, W = se.shape
    for dtype in (np.float64, np.float32):
        m = mean.astype(dtype)
        outs = {}
        for guided in (True, False):
            g = guides if guided else (None, None, None)
            got = renderer.denoise_pyramid(m, se, *g, SIGMAS, *window, levels)
            st = renderer.pyramid_stats()
            what = f"{name} {np.dtype(dtype).name} {window} L={levels} guided={guided}"
            assert got.dtype == m.dtype and got.shape == m.shape
            dr.check(got, pr.pyramid(m, se, *window, levels, *g, SIGMAS), what + " vs numpy")
            dr.check(got, rt.denoise_pyramid_host(m, se, *g, SIGMAS, *window, levels), what + " vs the host filter")
            assert np.array_equal(renderer.denoise_pyramid(m, se, *g, SIGMAS, *window, levels), got)   # repeats bit for bit
            assert st.kernel_ms > 0 and st.levels == levels and (st.radius, st.patch) == window[:2]
            assert (st.scratch_bytes == 0) == (levels == 1)
            assert st.scratch_bytes == _scratch(W, H, levels, dtype == np.float64, guided)
            if levels == 1:                                  # one level is the filter itself, bit for bit
                assert np.array_equal(got, renderer.denoise_guided(m, se, *g, SIGMAS, *window))
            outs[guided] = got
            print(f"{what}: kernel {st.kernel_ms:.3f} ms, scratch {st.scratch_bytes} B")
        assert not np.array_equal(outs[True], outs[False])                                   # the guides act


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("name", list(RENDERS))
def test_device_matches_numpy_and_host(rt, renderer, name, levels):
    _one(rt, renderer, name, levels, WINDOW)


def test_device_matches_numpy_and_host_at_the_widest_window(rt, renderer):
    _one(rt, renderer, "random_ragged", 3, (10, 3, 0.45))


def test_levels_act(rt, renderer):
    mean, se, *_ = ta._frame(rt, renderer, "cornell")
    outs = [renderer.denoise_pyramid(mean, se, None, None, None, SIGMAS, *WINDOW, L) for L in (1, 2, 3)]
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])


def test_a_small_frame_reuses_the_scratch_of_a_large_one(rt, renderer):
    """On a context of its own: the 40 x 40 frame allocates the scratch, the 9 x 5 frame after it fits
    in it (other offsets, the same allocation) and still matches; then the large frame again."""
    own = rt.Renderer(0)
    try:
        for name in ("cornell", "random_tiny", "cornell"):
            mean, se, *g = ta._frame(rt, renderer, name)
            H, W = se.shape
            got = own.denoise_pyramid(mean, se, *g, SIGMAS, *WINDOW, 3)
            assert own.pyramid_stats().scratch_bytes == _scratch(W, H, 3, True, True)
            dr.check(got, pr.pyramid(mean, se, *WINDOW, 3, *g, SIGMAS), f"{name} on a reused scratch vs numpy")
            assert np.array_equal(got, renderer.denoise_pyramid(mean, se, *g, SIGMAS, *WINDOW, 3))
    finally:
        own.close()


@pytest.mark.parametrize("name,fmt", [("random_counts", "f64"), ("random_ragged", "f32")])
def test_device_pointer_chain_is_the_host_pointer_chain(rt, renderer, name, fmt):
    """rt_render_adaptive, rt_render_features and rt_denoise_pyramid into torch tensors on one torch
    stream, no host round trip, against the same three calls on host arrays: the same bits."""
    import torch
    _, W, H, _, _, min_spp, step_spp, threshold = RENDERS[name]
    out_format, tdt = (rt.RT_OUT_F64, torch.float64) if fmt == "f64" else (rt.RT_OUT_F32, torch.float32)
    cam, p, pf = ta._setup(rt, renderer, name, out_format)
    mean_h, _, _, se_h = renderer.render_adaptive(cam, p, min_spp, step_spp, threshold)
    guides_h = renderer.render_features(cam, pf)
    want = renderer.denoise_pyramid(mean_h, se_h, *guides_h, SIGMAS, *WINDOW, 3)

    f64 = dict(dtype=torch.float64, device="cuda:0")
    mean_d = torch.zeros((H, W, 3), dtype=tdt, device="cuda:0")
    se_d, z_d = torch.zeros((H, W), **f64), torch.zeros((H, W), **f64)
    a_d, n_d = torch.zeros((H, W, 3), **f64), torch.zeros((H, W, 3), **f64)
    out_d = torch.full((H, W, 3), 7.0, dtype=tdt, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    s = stream.cuda_stream
    renderer.render_adaptive_device(cam, p, min_spp, step_spp, threshold, mean_d.data_ptr(), se_d.data_ptr(), stream=s)
    renderer.render_features_device(cam, pf, a_d.data_ptr(), n_d.data_ptr(), z_d.data_ptr(), stream=s)
    renderer.denoise_pyramid_device(mean_d.data_ptr(), se_d.data_ptr(), out_d.data_ptr(), W, H, a_d.data_ptr(),
                                    n_d.data_ptr(), z_d.data_ptr(), SIGMAS, out_format, *WINDOW, 3, stream=s)
    st = renderer.pyramid_stats()                         # waits for the kernels
    assert st.kernel_ms > 0 and st.levels == 3
    torch.cuda.synchronize()
    assert np.array_equal(out_d.cpu().numpy(), want)


def test_non_finite_pixels_behave_as_on_the_host(rt, renderer):
    mean, se, *guides = (np.array(x) for x in ta._frame(rt, renderer, "random_ragged"))
    mean[7, 11, 1] = np.nan
    se[15, 30] = np.inf
    for levels in (2, 3):
        for g in (guides, (None, None, None)):
            got = renderer.denoise_pyramid(mean, se, *g, SIGMAS, *WINDOW, levels)
            dr.check(got, rt.denoise_pyramid_host(mean, se, *g, SIGMAS, *WINDOW, levels), f"non-finite L={levels} vs host")
            dr.check(got, pr.pyramid(mean, se, *WINDOW, levels, *g, SIGMAS), f"non-finite L={levels} vs numpy")
            assert got[7, 11].tobytes() == mean[7, 11].tobytes() and got[15, 30].tobytes() == mean[15, 30].tobytes()
            assert np.isnan(got).sum() == 1


def test_invalid_arguments_leave_the_context_usable(rt, renderer):
    mean, se, a, n, z = ta._frame(rt, renderer, "random_tiny")
    want = renderer.denoise_pyramid(mean, se, a, n, z, SIGMAS, *WINDOW, 3)

    def still_filters():
        assert np.array_equal(renderer.denoise_pyramid(mean, se, a, n, z, SIGMAS, *WINDOW, 3), want)

    bad = [dict(levels=0), dict(levels=-1), dict(levels=6), dict(radius=0), dict(radius=11), dict(patch=-1), dict(patch=4),
           dict(k=0.0), dict(k=-1.0), dict(k=float("nan")), dict(k=float("inf")),
           dict(sigmas=(0.0, 0.2, 0.1)), dict(sigmas=(0.1, float("nan"), 0.1)), dict(sigmas=(0.1, 0.2, float("inf")))]
    for kw in bad:
        args = dict(sigmas=SIGMAS, radius=5, patch=2, k=1.0, levels=3)
        args.update(kw)
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
            renderer.denoise_pyramid(mean, se, a, n, z, **args)
        still_filters()
    m, s = np.ascontiguousarray(mean), np.ascontiguousarray(se)
    out = np.empty_like(m)
    lib = rt.load_library()
    par = lambda **kw: rt.PyramidParams(**{**dict(width=9, height=5, format=rt.RT_OUT_F64, on_device=0, radius=5,   # noqa: E731
                                                  patch=2, k=1.0, levels=3, reserved0=0, stream=None), **kw})
    ptr = lambda x: x.ctypes.data if x is not None else None   # noqa: E731
    calls = [(par(), m, s, m), (par(), None, s, out), (par(), m, None, out), (par(), m, s, None),   # out == mean, nulls
             (par(reserved0=1), m, s, out), (par(format=7), m, s, out), (par(width=0), m, s, out),
             (par(height=0), m, s, out)]
    for p, mm, ss, oo in calls:
        rc = lib.rt_denoise_pyramid(renderer.h, ctypes.byref(p), ptr(mm), ptr(ss), None, ptr(oo))
        assert rt.ERRORS.get(rc) == "RT_ERR_INVALID"
        still_filters()
    assert rt.ERRORS.get(lib.rt_denoise_pyramid(renderer.h, None, ptr(m), ptr(s), None, ptr(out))) == "RT_ERR_INVALID"
    assert rt.ERRORS.get(lib.rt_denoise_pyramid(None, ctypes.byref(par()), ptr(m), ptr(s), None, ptr(out))) == "RT_ERR_INVALID"
    still_filters()


def test_the_other_filters_keep_their_bits(rt, renderer):
    """rt_denoise and rt_denoise_guided on the same context before and after pyramid calls (which
    allocate and grow the context's scratch): the same bits."""
    mean, se, a, n, z = ta._frame(rt, renderer, "random_ragged")
    plain = renderer.denoise(mean, se, 5, 2, 1.0)
    guided = renderer.denoise_guided(mean, se, a, n, z, SIGMAS, 5, 2, 1.0)
    for levels in (2, 5):
        renderer.denoise_pyramid(mean, se, a, n, z, SIGMAS, *WINDOW, levels)
        assert np.array_equal(renderer.denoise(mean, se, 5, 2, 1.0), plain)
        assert np.array_equal(renderer.denoise_guided(mean, se, a, n, z, SIGMAS, 5, 2, 1.0), guided)
