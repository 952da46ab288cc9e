"""rt_denoise_host: the variance-guided NL-means filter of include/rt/rt_abi.h on the host (no
device), against the numpy restatement of tests/denoise_reference.py on frames derived from the CPU
oracle. Tolerances: that module's (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded reference in f32).
"""
import ctypes

import numpy as np
import pytest

from tests import denoise_reference as dr
from tests import oracle_binding as ob


@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
@pytest.mark.parametrize("name", dr.CPU_INPUTS)
def test_host_filter_matches_numpy(rt, name, radius, patch, k):
    """Cornell 40x40, the light scene (884 pixels with se = 0: delta up to 1e10 and more), ragged
    37x21, a 9x5 crop (at radius 10 the window is larger than the frame), tiles at mixed sample
    counts, and an f32 frame."""
    mean, se = dr.cpu_input(name)
    if name == "light":
        assert int((se == 0).sum()) == 884
    got = rt.denoise_host(mean, se, radius, patch, k)
    ref = dr.cpu_reference(name, radius, patch, k)
    assert got.dtype == mean.dtype and np.isfinite(got).all()
    dr.check(got, ref, f"{name} r={radius} f={patch} k={k}")
    assert not np.array_equal(got, mean)          # it did filter


@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
def test_nan_and_inf_stay_where_they_are(rt, radius, patch, k):
    """One NaN and one +Inf pixel: both come back unchanged, every other pixel is finite and equals
    the reference on the same input."""
    mean, se = (np.array(a) for a in dr.cpu_input("random_ragged"))
    mean[7, 11] = np.nan
    mean[15, 30, 1] = np.inf
    got = rt.denoise_host(mean, se, radius, patch, k)
    assert np.isnan(got[7, 11]).all()
    assert np.array_equal(got[15, 30], mean[15, 30])
    rest = np.ones(mean.shape[:2], dtype=bool)
    rest[7, 11] = rest[15, 30] = False
    assert np.isfinite(got[rest]).all()
    ref = dr.denoise(mean, se, radius, patch, k)
    dr.check(got[rest], ref[rest], f"NaN / Inf frame r={radius} f={patch}")
    # a non-finite error estimate keeps its pixel too
    se[3, 4], se[9, 2] = np.inf, np.nan
    got = rt.denoise_host(mean, se, radius, patch, k)
    assert np.array_equal(got[3, 4], mean[3, 4]) and np.array_equal(got[9, 2], mean[9, 2])
    rest[3, 4] = rest[9, 2] = False
    assert np.isfinite(got[rest]).all()
    dr.check(got[rest], dr.denoise(mean, se, radius, patch, k)[rest], f"NaN / Inf map r={radius} f={patch}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constant_frame_is_unchanged(rt, dtype):
    """A constant frame with se = 0: every delta is 0 and every weight 1, so out = (n c) / n. With
    dyadic channel values the sums of up to 441 equal terms are exact and the frame comes back bit
    for bit; with values f64 does not hold exactly (0.3, 0.7, 0.1) the sum n c rounds, and the frame
    comes back within the tolerance."""
    se = np.zeros((21, 37))
    mean = np.empty((21, 37, 3), dtype=dtype)
    for radius, patch, k in dr.PARAMS:
        mean[...] = np.array([0.25, 0.75, 3.5], dtype=dtype)
        assert np.array_equal(rt.denoise_host(mean, se, radius, patch, k), mean)
        mean[...] = np.array([0.3, 0.7, 0.1], dtype=dtype)
        dr.check(rt.denoise_host(mean, se, radius, patch, k), mean, f"constant frame r={radius} f={patch}")


def test_quality_on_the_cornell_box(rt):
    """Cornell 40x40 at 16 spp, (3, 1, 0.45), against the oracle at 2048 spp: the reference's own
    linear-RMSE ratio after / before is at most 0.6 (0.48 measured), and so is the library's."""
    mean, se = dr.cpu_input("cornell")
    truth = ob.render(5, 40, 40, 2048)
    before = dr.rmse(mean, truth)
    ref_ratio = dr.rmse(dr.cpu_reference("cornell", 3, 1, 0.45), truth) / before
    print(f"RMSE before {before:.4f}, numpy reference after / before {ref_ratio:.3f}")
    assert ref_ratio <= 0.6
    lib_ratio = dr.rmse(rt.denoise_host(mean, se, 3, 1, 0.45), truth) / before
    print(f"library after / before {lib_ratio:.3f}")
    assert lib_ratio <= 0.6


def _raw(rt, params, mean, se, out):
    p = lambda a: a.ctypes.data if a is not None else None   # noqa: E731
    return rt.load_library().rt_denoise_host(ctypes.byref(params) if params is not None else None, p(mean), p(se), p(out))


def test_invalid_arguments(rt):
    W, H = 12, 7
    mean, se, out = np.ones((H, W, 3)), np.zeros((H, W)), np.empty((H, W, 3))
    ok = lambda **kw: rt.DenoiseParams(**{**dict(width=W, height=H, format=rt.RT_OUT_F64, on_device=0, radius=3,   # noqa: E731
                                                 patch=1, k=0.45, stream=None), **kw})
    assert _raw(rt, ok(), mean, se, out) == rt.RT_OK
    bad = [(None, mean, se, out), (ok(), None, se, out), (ok(), mean, None, out), (ok(), mean, se, None),
           (ok(), mean, se, mean)]                                            # null pointers, out == mean
    bad += [(ok(**kw), mean, se, out) for kw in (
        dict(format=2), dict(format=-1), dict(width=0), dict(height=0), dict(width=-3), dict(radius=0), dict(radius=11),
        dict(patch=-1), dict(patch=4), dict(k=0.0), dict(k=-1.0), dict(k=float("inf")), dict(k=float("nan")))]
    for args in bad:
        assert rt.ERRORS.get(_raw(rt, *args)) == "RT_ERR_INVALID", args
        assert rt.load_library().rt_last_error()                              # and says why
    for kw in (dict(radius=0), dict(patch=4), dict(k=0.0)):                   # the wrapper raises
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
            rt.denoise_host(mean, se, **{**dict(radius=3, patch=1, k=0.45), **kw})
    with pytest.raises(rt.RTError):
        rt.denoise_host(mean, se[:, :5])
