"""rt_denoise_guided on the device: rt_denoise with feature guides in its weights
(include/rt/rt_abi.h).

Every case filters the library's own rt_render_adaptive frame with the library's own
rt_render_features buffers at 8 spp as guides (tests/test_gpu_adaptive.py and
tests/test_gpu_features.py hold those to their references); the numpy restatement of
tests/denoise_guided_reference.py and rt_denoise_guided_host run on the same arrays. Tolerances:
tests/denoise_reference.py's (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded reference in f32).
The frames are tests/test_gpu_denoise.py's.
"""
import numpy as np
import pytest

from tests import denoise_guided_reference as gr
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
    """(mean f64, se, albedo, normal, depth) of one adaptive render and one feature pass, rendered once."""
    if name not in _frames:
        cam, p, pf = _setup(rt, renderer, name)
        _, _, _, _, _, min_spp, step_spp, threshold = RENDERS[name]
        mean, _, _, se = renderer.render_adaptive(cam, p, min_spp, step_spp, threshold)
        guides = renderer.render_features(cam, pf)
        for a in (mean, se, *guides):
            assert np.isfinite(a).all()
            a.setflags(write=False)
        assert guides[2].max() > 0
        _frames[name] = (mean, se, *guides)
    return _frames[name]


@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
@pytest.mark.parametrize("name", list(RENDERS))
def test_device_guided_matches_numpy_and_host(rt, renderer, name, radius, patch, k):
    mean, se, a, n, z = _frame(rt, renderer, name)
    for dtype in (np.float64, np.float32):
        m = mean.astype(dtype)
        got = renderer.denoise_guided(m, se, a, n, z, SIGMAS, radius, patch, k)
        st = renderer.denoise_stats()
        what = f"{name} {np.dtype(dtype).name} r={radius} f={patch} k={k}"
        assert got.dtype == m.dtype and got.shape == m.shape
        dr.check(got, gr.denoise_guided(m, se, radius, patch, k, a, n, z, SIGMAS), what + " vs numpy")
        dr.check(got, rt.denoise_guided_host(m, se, a, n, z, SIGMAS, radius, patch, k), what + " vs the host filter")
        assert np.array_equal(renderer.denoise_guided(m, se, a, n, z, SIGMAS, radius, patch, k), got)   # repeats bit for bit
        assert st.kernel_ms > 0 and 0 < st.lds_bytes <= 65536 and (st.radius, st.patch) == (radius, patch)
        plain = renderer.denoise(m, se, radius, patch, k)
        assert np.array_equal(renderer.denoise_guided(m, se, None, None, None, SIGMAS, radius, patch, k), plain)
        assert not np.array_equal(got, plain)                                   # the guides act
        print(f"{what}: kernel {st.kernel_ms:.3f} ms, LDS {st.lds_bytes} B")


@pytest.mark.parametrize("subset", [(0,), (1,), (2,), (0, 2)])
def test_guide_subsets(rt, renderer, subset):
    mean, se, *guides = _frame(rt, renderer, "random_ragged")
    a, n, z = (g if i in subset else None for i, g in enumerate(guides))
    got = renderer.denoise_guided(mean, se, a, n, z, SIGMAS, 5, 2, 1.0)
    dr.check(got, gr.denoise_guided(mean, se, 5, 2, 1.0, a, n, z, SIGMAS), f"guides {subset}")


@pytest.mark.parametrize("name,fmt", [("random_counts", "f64"), ("random_ragged", "f32")])
def test_device_pointer_chain_is_the_host_pointer_chain(rt, renderer, name, fmt):
    """rt_render_adaptive, rt_render_features and rt_denoise_guided into torch tensors on one torch
    stream, no host round trip, against the same three calls on host arrays: the same bits."""
    import torch
    _, W, H, _, _, min_spp, step_spp, threshold = RENDERS[name]
    out_format, tdt = (rt.RT_OUT_F64, torch.float64) if fmt == "f64" else (rt.RT_OUT_F32, torch.float32)
    cam, p, pf = _setup(rt, renderer, name, out_format)
    mean_h, _, _, se_h = renderer.render_adaptive(cam, p, min_spp, step_spp, threshold)
    guides_h = renderer.render_features(cam, pf)
    want = renderer.denoise_guided(mean_h, se_h, *guides_h, SIGMAS, 10, 3, 0.45)

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
    renderer.denoise_guided_device(mean_d.data_ptr(), se_d.data_ptr(), out_d.data_ptr(), W, H, a_d.data_ptr(),
                                   n_d.data_ptr(), z_d.data_ptr(), SIGMAS, out_format, 10, 3, 0.45, stream=s)
    assert renderer.denoise_stats().kernel_ms > 0          # waits for the kernel
    torch.cuda.synchronize()
    for got, ref in zip((a_d, n_d, z_d), guides_h):
        assert np.array_equal(got.cpu().numpy(), ref)
    assert np.array_equal(out_d.cpu().numpy(), want)


def test_nan_feature_pixel_behaves_as_on_the_host(rt, renderer):
    mean, se, a, n, z = (np.array(x) for x in _frame(rt, renderer, "random_ragged"))
    a[7, 11, 1] = np.nan
    n[15, 30] = np.inf
    z[3, 4] = np.nan
    for radius, patch, k in dr.PARAMS[:2]:
        got = renderer.denoise_guided(mean, se, a, n, z, SIGMAS, radius, patch, k)
        assert np.isfinite(got).all()
        dr.check(got, rt.denoise_guided_host(mean, se, a, n, z, SIGMAS, radius, patch, k), f"NaN feature r={radius} vs host")
        dr.check(got, gr.denoise_guided(mean, se, radius, patch, k, a, n, z, SIGMAS), f"NaN feature r={radius} vs numpy")
        for q in ((7, 11), (15, 30), (3, 4)):
            assert np.array_equal(got[q], mean[q])


def test_invalid_guides(rt, renderer):
    mean, se, a, n, z = _frame(rt, renderer, "random_tiny")
    for sig in ((0.0, 0.2, 0.1), (0.1, float("nan"), 0.1), (0.1, 0.2, float("inf")), (-1.0, 0.2, 0.1)):
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
            renderer.denoise_guided(mean, se, a, n, z, sig, 3, 1, 0.45)
    # the sigma of a guide left out is ignored, and the context still filters
    got = renderer.denoise_guided(mean, se, a, None, z, (0.1, float("nan"), 0.1), 3, 1, 0.45)
    dr.check(got, gr.denoise_guided(mean, se, 3, 1, 0.45, a, None, z, SIGMAS), "after the errors")
