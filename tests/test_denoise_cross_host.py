"""rt_denoise_cross_host: the cross-filtered NL-means of include/rt/rt_abi.h on the host (no
device), against the numpy restatement of tests/denoise_cross_reference.py on half frames derived
from the CPU oracle's samples by parity, and the identities the contract states. Tolerances:
denoise_reference.check's (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded reference in f32), for
out and for stderr_out.
"""
import ctypes

import numpy as np
import pytest

from tests import denoise_cross_reference as cr
from tests import denoise_guided_reference as gr
from tests import denoise_reference as dr
from tests import oracle_binding as ob


def _guides(name, guided):
    if not guided:
        return {}
    al, no, de = gr.cpu_guides(dr.cpu_input(name)[0])
    return dict(albedo=al, normal=no, depth=de, sigmas=gr.SIGMAS)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
@pytest.mark.parametrize("name", dr.CPU_INPUTS)
def test_host_filter_matches_numpy(rt, name, radius, patch, k, guided):
    """denoise_reference.cpu_input's frames split by sample parity, scale 2, with and without guides:
    out and stderr_out against the reference."""
    a, b, se = cr.cpu_input(name)
    got, got_se = rt.denoise_cross_host(a, b, se, radius=radius, patch=patch, k=k, variance_scale=cr.SCALE,
                                        **_guides(name, guided))
    ref, ref_se = cr.cpu_reference(name, radius, patch, k, guided)
    what = f"{name} r={radius} f={patch} k={k} guided={guided}"
    assert got.dtype == a.dtype and np.isfinite(got).all() and np.isfinite(got_se).all()
    dr.check(got, ref, what)
    dr.check(got_se, ref_se, what + " stderr_out")
    assert not np.array_equal(got.astype(np.float64), 0.5 * (a.astype(np.float64) + b))   # it did filter
    # without stderr_out: the same frame
    only, none = rt.denoise_cross_host(a, b, se, radius=radius, patch=patch, k=k, variance_scale=cr.SCALE,
                                       want_stderr=False, **_guides(name, guided))
    assert none is None and np.array_equal(only, got)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
@pytest.mark.parametrize("name", dr.CPU_INPUTS)
def test_same_halves_are_the_plain_filter(rt, name, radius, patch, k, guided):
    """mean_a = mean_b = M at scale 1: rt_denoise_host(M, se) (guided: rt_denoise_guided_host) bit for
    bit, and stderr_out is 0 everywhere."""
    mean, se = dr.cpu_input(name)
    g = _guides(name, guided)
    got, got_se = rt.denoise_cross_host(mean, mean, se, radius=radius, patch=patch, k=k, variance_scale=1.0, **g)
    plain = rt.denoise_guided_host(mean, se, radius=radius, patch=patch, k=k, **g) if guided else \
        rt.denoise_host(mean, se, radius, patch, k)
    assert got.dtype == plain.dtype and got.tobytes() == plain.tobytes()
    assert np.array_equal(got_se, np.zeros_like(se))


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("radius,patch,k", dr.PARAMS[:3])
def test_swapping_the_halves_changes_no_bit(rt, radius, patch, k, guided):
    for name in ("random_ragged", "cornell_f32"):
        a, b, se = cr.cpu_input(name)
        g = _guides(name, guided)
        o1, s1 = rt.denoise_cross_host(a, b, se, radius=radius, patch=patch, k=k, variance_scale=cr.SCALE, **g)
        o2, s2 = rt.denoise_cross_host(b, a, se, radius=radius, patch=patch, k=k, variance_scale=cr.SCALE, **g)
        assert o1.tobytes() == o2.tobytes() and s1.tobytes() == s2.tobytes()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constant_frame_is_unchanged(rt, dtype):
    """Constant halves with se = 0 and dyadic channel values: every delta is 0, every weight 1, the
    sums of up to 441 equal terms are exact, and the frame comes back bit for bit with stderr_out 0."""
    se = np.zeros((21, 37))
    mean = np.empty((21, 37, 3), dtype=dtype)
    mean[...] = np.array([0.25, 0.75, 3.5], dtype=dtype)
    for radius, patch, k in dr.PARAMS:
        out, so = rt.denoise_cross_host(mean, mean.copy(), se, radius=radius, patch=patch, k=k, variance_scale=cr.SCALE)
        assert np.array_equal(out, mean) and np.array_equal(so, se)


@pytest.mark.parametrize("radius,patch,k", dr.PARAMS)
@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_one_bad_half_makes_the_pixel_bad(rt, radius, patch, k, value):
    """A NaN or Inf in one half at one pixel: out there is 0.5 (M_A + M_B), and no other pixel's out
    or stderr_out differs from the run where that pixel is bad in both halves. The reference agrees."""
    a, b, se = (np.array(x) for x in cr.cpu_input("random_ragged"))
    y, x = 7, 11
    a[y, x, 1] = value
    both = b.copy()
    both[y, x, 1] = value
    o1, s1 = rt.denoise_cross_host(a, b, se, radius=radius, patch=patch, k=k, variance_scale=cr.SCALE)
    o2, s2 = rt.denoise_cross_host(a, both, se, radius=radius, patch=patch, k=k, variance_scale=cr.SCALE)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(o1[y, x], 0.5 * (a[y, x] + b[y, x]), equal_nan=True)
    rest = np.ones(se.shape, dtype=bool)
    rest[y, x] = False
    assert np.isfinite(o1[rest]).all() and o1[rest].tobytes() == o2[rest].tobytes()
    far = np.ones(se.shape, dtype=bool)              # stderr_out's 3 x 3 reaches the bad pixel's e
    far[y - 1:y + 2, x - 1:x + 2] = False
    assert s1[far].tobytes() == s2[far].tobytes()
    ref, ref_se = cr.denoise_cross(a, b, se, radius, patch, k, cr.SCALE)
    dr.check(o1[rest], ref[rest], f"bad pixel r={radius} f={patch}")
    dr.check(s1, ref_se, f"bad pixel r={radius} f={patch} stderr_out")
    # a non-finite error estimate makes its pixel bad too
    se[3, 4], se[9, 2] = np.inf, np.nan
    o3, s3 = rt.denoise_cross_host(a, b, se, radius=radius, patch=patch, k=k, variance_scale=cr.SCALE)
    for q in ((3, 4), (9, 2)):
        assert np.array_equal(o3[q], 0.5 * (a[q] + b[q]))
        rest[q] = False
    assert np.isfinite(o3[rest]).all()
    ref, ref_se = cr.denoise_cross(a, b, se, radius, patch, k, cr.SCALE)
    dr.check(o3[rest], ref[rest], f"bad map r={radius} f={patch}")
    dr.check(s3, ref_se, f"bad map r={radius} f={patch} stderr_out")


def _quality(out, se_out, truth):
    from tests import adaptive_reference as ar
    y_rmse = dr.rmse(ar.luma(np.asarray(out, dtype=np.float64)), ar.luma(truth))
    return dr.rmse(out, truth), float(np.sqrt(np.mean(se_out ** 2))) / y_rmse


def test_quality_and_honesty_on_the_cornell_box(rt):
    """Cornell 40x40 at 16 spp, (3, 1, 0.45), scale 2, against the oracle at 2048 spp, on the numpy
    reference first and then on the library: linear RMSE after / before at most 0.6
    (test_quality_on_the_cornell_box's bound), and rms(stderr_out) / RMSE of Y(out) within
    [0.5, 1.25]."""
    a, b, se = cr.cpu_input("cornell")
    mean, _ = dr.cpu_input("cornell")
    truth = ob.render(5, 40, 40, 2048)
    before = dr.rmse(mean, truth)
    ref_rmse, ref_honesty = _quality(*cr.cpu_reference("cornell", 3, 1, 0.45, False), truth)
    print(f"RMSE before {before:.4f}; numpy reference after / before {ref_rmse / before:.3f}, "
          f"rms(stderr_out) / RMSE(Y(out)) {ref_honesty:.3f}")
    assert ref_rmse / before <= 0.6 and 0.5 <= ref_honesty <= 1.25
    lib_rmse, lib_honesty = _quality(*rt.denoise_cross_host(a, b, se, radius=3, patch=1, k=0.45, variance_scale=2.0),
                                     truth)
    print(f"library after / before {lib_rmse / before:.3f}, rms(stderr_out) / RMSE(Y(out)) {lib_honesty:.3f}")
    assert lib_rmse / before <= 0.6 and 0.5 <= lib_honesty <= 1.25


def _raw(rt, params, a, b, se, g, out, se_out):
    p = lambda x: x.ctypes.data if x is not None else None   # noqa: E731
    return rt.load_library().rt_denoise_cross_host(ctypes.byref(params) if params is not None else None, p(a), p(b),
                                                   p(se), ctypes.byref(g) if g is not None else None, p(out), p(se_out))


def test_invalid_arguments(rt):
    W, H = 12, 7
    a, b, se = np.ones((H, W, 3)), np.ones((H, W, 3)), np.zeros((H, W))
    out, so = np.empty((H, W, 3)), np.empty((H, W))
    ok = lambda **kw: rt.CrossParams(**{**dict(width=W, height=H, format=rt.RT_OUT_F64, on_device=0, radius=3,   # noqa: E731
                                               patch=1, k=0.45, variance_scale=2.0, stream=None), **kw})
    assert _raw(rt, ok(), a, b, se, None, out, so) == rt.RT_OK
    assert _raw(rt, ok(), a, b, se, None, out, None) == rt.RT_OK            # stderr_out may be null
    assert _raw(rt, ok(), a, a, se, None, out, so) == rt.RT_OK              # and the halves may be one frame
    bad = [(None, a, b, se, None, out, so), (ok(), None, b, se, None, out, so), (ok(), a, None, se, None, out, so),
           (ok(), a, b, None, None, out, so), (ok(), a, b, se, None, None, so),
           (ok(), a, b, se, None, a, so), (ok(), a, b, se, None, b, so),    # out aliases an input
           (ok(), a, b, se, None, out, se)]                                 # stderr_out == stderr_map
    bad += [(ok(**kw), a, b, se, None, out, so) for kw in (
        dict(format=2), dict(format=-1), dict(width=0), dict(height=0), dict(width=-3), dict(radius=0), dict(radius=11),
        dict(patch=-1), dict(patch=4), dict(k=0.0), dict(k=-1.0), dict(k=float("inf")), dict(k=float("nan")),
        dict(variance_scale=0.0), dict(variance_scale=-2.0), dict(variance_scale=float("inf")),
        dict(variance_scale=float("nan")))]
    for sig in (0.0, -1.0, float("nan"), float("inf")):                     # a guide given with a bad sigma
        bad.append((ok(), a, b, se, rt.DenoiseGuides(None, None, se.ctypes.data, 1.0, 1.0, sig), out, so))
    for args in bad:
        assert rt.ERRORS.get(_raw(rt, *args)) == "RT_ERR_INVALID", args
        assert rt.load_library().rt_last_error()                            # and says why
    assert _raw(rt, ok(), a, b, se, rt.DenoiseGuides(None, None, None, 0.0, 0.0, 0.0), out, so) == rt.RT_OK
    for kw in (dict(radius=0), dict(patch=4), dict(k=0.0), dict(variance_scale=0.0)):   # the wrapper raises
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
            rt.denoise_cross_host(a, b, se, **{**dict(radius=3, patch=1, k=0.45), **kw})
    with pytest.raises(rt.RTError):
        rt.denoise_cross_host(a, b[:, :5], se)
    with pytest.raises(rt.RTError):
        rt.denoise_cross_host(a, b.astype(np.float32), se)
