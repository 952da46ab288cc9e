"""rt_denoise_guided_host: the feature-guided NL-means filter of include/rt/rt_abi.h on the host (no
device), against the numpy restatement of tests/denoise_guided_reference.py, under
tests/denoise_reference.py's tolerances (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded
reference in f32). The frames are denoise_reference.cpu_input's; the guides are made from the frame
and a fixed-seed generator (denoise_guided_reference.cpu_guides).
"""
import ctypes
import itertools

import numpy as np
import pytest

from tests import denoise_guided_reference as gr
from tests import denoise_reference as dr

INPUTS = ["cornell", "random_ragged", "crop", "cornell_f32"]
SUBSETS = [s for n in (1, 2, 3) for s in itertools.combinations(range(3), n)]   # the 7 non-empty subsets
# every subset of guides at one parameter set, all three guides at the others
CASES = [(dr.PARAMS[0], s) for s in SUBSETS] + [(p, (0, 1, 2)) for p in dr.PARAMS[1:]]


def _pick(guides, subset):
    return [g if i in subset else None for i, g in enumerate(guides)]


@pytest.mark.parametrize("params,subset", CASES, ids=lambda v: "-".join(str(x) for x in v))
@pytest.mark.parametrize("name", INPUTS)
def test_host_guided_matches_numpy(rt, name, params, subset):
    radius, patch, k = params
    mean, se = dr.cpu_input(name)
    a, n, z = _pick(gr.cpu_guides(mean), subset)
    got = rt.denoise_guided_host(mean, se, a, n, z, gr.SIGMAS, radius, patch, k)
    ref = gr.denoise_guided(mean, se, radius, patch, k, a, n, z, gr.SIGMAS)
    assert got.dtype == mean.dtype and np.isfinite(got).all()
    dr.check(got, ref, f"{name} r={radius} f={patch} k={k} guides {subset}")
    # the guides act: the result is not the plain filter's
    assert not np.array_equal(got, rt.denoise_host(mean, se, radius, patch, k))


@pytest.mark.parametrize("name", INPUTS)
def test_no_guides_is_the_plain_filter(rt, name):
    """No guide frames, through the wrapper's guides struct and through g == NULL: rt_denoise_host's
    bits; the sigmas of absent guides (0, NaN, negative) are ignored."""
    mean, se = dr.cpu_input(name)
    for radius, patch, k in dr.PARAMS:
        plain = rt.denoise_host(mean, se, radius, patch, k)
        assert np.array_equal(rt.denoise_guided_host(mean, se, None, None, None, (0.0, float("nan"), -1.0), radius,
                                                     patch, k), plain)
        m = np.ascontiguousarray(mean)
        s = np.ascontiguousarray(se)
        out = np.empty_like(m)
        p = rt.DenoiseParams(m.shape[1], m.shape[0], rt.RT_OUT_F64 if m.dtype == np.float64 else rt.RT_OUT_F32, 0,
                             radius, patch, k, None)
        assert rt.load_library().rt_denoise_guided_host(ctypes.byref(p), m.ctypes.data, s.ctypes.data, None,
                                                        out.ctypes.data) == rt.RT_OK
        assert np.array_equal(out, plain)


def test_albedo_edge_is_kept(rt):
    """A 24x16 frame, left half 0.2 and right half 0.8 in every channel, se = 1, k = 0.45, patch 1,
    radius 3. Unguided: every delta is (d^2 - 2) / (1e-10 + 2 k^2) with d^2 <= 0.36, negative, so
    every colour weight is exp(-0) = 1 and the filter is a box blur: the columns next to the edge
    move by more than 0.1 towards the other side (4 of the row's 7 neighbours are their own
    side's: 3/7 x 0.6 = 0.257). With albedo = the frame and sigma_albedo = 0.1, Phi across the edge
    is 3 x 0.36 / 0.01 = 108 and within a side 0: the weights across are exp(-108) = 1e-47, and the
    output equals the input within 1e-12."""
    W, H = 24, 16
    mean = np.full((H, W, 3), 0.2)
    mean[:, W // 2:] = 0.8
    se = np.ones((H, W))
    plain = rt.denoise_host(mean, se, 3, 1, 0.45)
    assert (plain[:, W // 2 - 1] - 0.2 > 0.1).all() and (0.8 - plain[:, W // 2] > 0.1).all()
    guided = rt.denoise_guided_host(mean, se, albedo=mean, sigmas=(0.1, 1.0, 1.0), radius=3, patch=1, k=0.45)
    err = float(np.max(np.abs(guided - mean)))
    print(f"guided: max |out - in| = {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_feature_removes_only_its_pairs(rt, bad):
    """A NaN or Inf feature value at q: Phi of every pair that touches q is not finite, so q gets
    only its own weight 1 (out(q) = M(q) within rounding) and contributes to no other pixel; every
    output pixel is finite and matches numpy."""
    mean, se = dr.cpu_input("random_ragged")
    a, n, z = (np.array(g) for g in gr.cpu_guides(mean))
    a[7, 11, 1] = bad
    n[15, 30, 0] = bad
    z[3, 4] = bad
    for radius, patch, k in dr.PARAMS[:2]:
        got = rt.denoise_guided_host(mean, se, a, n, z, gr.SIGMAS, radius, patch, k)
        ref = gr.denoise_guided(mean, se, radius, patch, k, a, n, z, gr.SIGMAS)
        assert np.isfinite(got).all()
        dr.check(got, ref, f"feature {bad} r={radius} f={patch}")
        for q in ((7, 11), (15, 30), (3, 4)):
            assert np.allclose(got[q], mean[q], rtol=1e-15, atol=0)
        # and q's value reaches no neighbour: the same result with another colour at q
        m2 = np.array(mean)
        m2[7, 11] = m2[7, 11] + 5.0
        got2 = rt.denoise_guided_host(m2, se, a, n, z, gr.SIGMAS, radius, 0, k)
        got0 = rt.denoise_guided_host(mean, se, a, n, z, gr.SIGMAS, radius, 0, k)
        rest = np.ones(mean.shape[:2], dtype=bool)
        rest[7, 11] = False
        assert np.array_equal(got2[rest], got0[rest])


def _raw(rt, params, mean, se, guides, out):
    p = lambda x: x.ctypes.data if x is not None else None   # noqa: E731
    return rt.load_library().rt_denoise_guided_host(ctypes.byref(params), p(mean), p(se),
                                                    ctypes.byref(guides) if guides is not None else None, p(out))


def test_invalid_arguments(rt):
    W, H = 12, 7
    mean, se, out = np.ones((H, W, 3)), np.zeros((H, W)), np.empty((H, W, 3))
    a, n, z = np.ones((H, W, 3)), np.ones((H, W, 3)), np.ones((H, W))
    params = rt.DenoiseParams(W, H, rt.RT_OUT_F64, 0, 3, 1, 0.45, None)
    guides = lambda sig, use=(1, 1, 1): rt.DenoiseGuides(   # noqa: E731
        *(g.ctypes.data if u else None for g, u in zip((a, n, z), use)), *sig)
    assert _raw(rt, params, mean, se, guides((0.1, 0.2, 0.3)), out) == rt.RT_OK
    for v in (0.0, -0.5, float("nan"), float("inf")):
        for i in range(3):
            sig = [0.1, 0.2, 0.3]
            sig[i] = v
            assert rt.ERRORS.get(_raw(rt, params, mean, se, guides(sig), out)) == "RT_ERR_INVALID", (v, i)
            assert rt.load_library().rt_last_error()
            use = [1, 1, 1]
            use[i] = 0                                       # the sigma of a NULL guide is ignored
            assert _raw(rt, params, mean, se, guides(sig, use), out) == rt.RT_OK, (v, i)
    assert rt.ERRORS.get(_raw(rt, params, mean, se, guides((0.1, 0.2, 0.3)), mean)) == "RT_ERR_INVALID"   # out == mean
    bad_params = rt.DenoiseParams(W, H, rt.RT_OUT_F64, 0, 11, 1, 0.45, None)
    assert rt.ERRORS.get(_raw(rt, bad_params, mean, se, guides((0.1, 0.2, 0.3)), out)) == "RT_ERR_INVALID"
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
        rt.denoise_guided_host(mean, se, albedo=a, sigmas=(0.0, 1.0, 1.0))
    with pytest.raises(rt.RTError):
        rt.denoise_guided_host(mean, se, depth=z[:, :5])
