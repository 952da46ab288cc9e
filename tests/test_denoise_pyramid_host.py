"""rt_denoise_pyramid_host: the multi-scale NL-means filter of include/rt/rt_abi.h on the host (no
device), against the numpy restatement of tests/denoise_pyramid_reference.py, under
tests/denoise_reference.py's tolerances (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded reference
in f32). The frames are denoise_reference.cpu_input's and five odd sizes (1 x 1, 2 x 1, 3 x 3, 9 x 5,
72 x 9: blocks of one and two pixels and clamped taps on both axes), f64 and f32; the guides come
from pixel coordinates (denoise_atrous_reference.coord_guides).
"""
import ctypes

import numpy as np
import pytest

from tests import denoise_pyramid_reference as pr
from tests import denoise_reference as dr


def _run(rt, mean, se, params, levels, guided):
    return rt.denoise_pyramid_host(mean, se, *pr.guides_for(mean, guided), pr.SIGMAS, *params, levels)


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("params", pr.PARAMS, ids=lambda p: "r%d_f%d_k%g" % p)
@pytest.mark.parametrize("levels", pr.LEVELS)
@pytest.mark.parametrize("name", pr.CPU_FRAMES)
def test_host_matches_numpy(rt, name, levels, params, guided):
    mean, se = pr.cpu_frame(name)
    out = _run(rt, mean, se, params, levels, guided)
    ref = pr.cpu_reference(name, *params, levels, guided)
    assert out.dtype == mean.dtype and out.shape == mean.shape and np.isfinite(out).all()
    dr.check(out, ref, f"{name} L={levels} {params} guided={guided}")
    if levels == 1:                                          # one level is the filter itself, bit for bit
        plain = rt.denoise_guided_host(mean, se, *pr.guides_for(mean, guided), pr.SIGMAS, *params)
        assert np.array_equal(out, plain)
    elif mean.shape[0] * mean.shape[1] >= 45:
        assert not np.array_equal(out, pr.cpu_reference(name, *params, 1, guided))   # the coarse levels act


def test_no_guides_is_all_null_guides(rt):
    mean, se = dr.cpu_input("random_ragged")
    m, s = np.ascontiguousarray(mean), np.ascontiguousarray(se)
    for levels in (1, 3):
        out = _run(rt, mean, se, (3, 1, 0.45), levels, False)
        raw = np.empty_like(m)
        p = rt.PyramidParams(m.shape[1], m.shape[0], rt.RT_OUT_F64, 0, 3, 1, 0.45, levels, 0, None)
        assert rt.load_library().rt_denoise_pyramid_host(ctypes.byref(p), m.ctypes.data, s.ctypes.data, None,
                                                         raw.ctypes.data) == rt.RT_OK
        assert np.array_equal(raw, out)
        # the sigmas of NULL guides are ignored
        assert np.array_equal(rt.denoise_pyramid_host(mean, se, None, None, None, (0.0, float("nan"), -1.0), 3, 1, 0.45,
                                                      levels), out)


def _dilate(t, d):
    """t (H, W) bool grown by d pixels (Chebyshev)."""
    H, W = t.shape
    out = np.zeros_like(t)
    for y, x in zip(*np.nonzero(t)):
        out[max(0, y - d):y + d + 1, max(0, x - d):x + d + 1] = True
    return out


def _reach(shape, bad, radius, patch, levels):
    """The level-0 pixels whose output can depend on the pixel `bad` = (y, x): the data flow of the
    contract, followed with booleans. Down: a block that holds a reached pixel is reached. A level's
    filter reads p's window and the patches around both ends of every pair: everything within
    radius + patch of p. Up: K(c) is reached if R_{l+1}(c) or a pixel of c's block of D_l is; R_l(p)
    if D_l(p) or one of p's four taps is."""
    t = np.zeros(shape, dtype=bool)
    t[bad] = True
    C = [t]
    for _ in range(levels - 1):
        H, W = C[-1].shape
        pad = np.zeros((2 * ((H + 1) // 2), 2 * ((W + 1) // 2)), dtype=bool)
        pad[:H, :W] = C[-1]
        C.append(pad[0::2, 0::2] | pad[0::2, 1::2] | pad[1::2, 0::2] | pad[1::2, 1::2])
    D = [_dilate(c, radius + patch) for c in C]
    R = D[-1]
    for l in range(levels - 2, -1, -1):
        H, W = D[l].shape
        hc, wc = R.shape
        pad = np.zeros((2 * hc, 2 * wc), dtype=bool)
        pad[:H, :W] = D[l]
        K = R | pad[0::2, 0::2] | pad[0::2, 1::2] | pad[1::2, 0::2] | pad[1::2, 1::2]
        cx, ox = pr.tap_coords(W, wc)
        cy, oy = pr.tap_coords(H, hc)
        R = D[l].copy()
        for ty, tx in ((cy, cx), (cy, ox), (oy, cx), (oy, ox)):
            R |= K[ty[:, None], tx[None, :]]
    return R


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("what", ["nan_mean", "inf_se"])
def test_a_non_finite_pixel_stays_and_reaches_only_what_reads_it(rt, what, dtype):
    """17 x 16 at L = 3 (levels of 17 x 16, 9 x 8, 5 x 4; column 16 has blocks of two pixels) with a
    window of radius 1, patch 0, small enough for part of the frame to lie outside the bad pixel's
    reach at every level: the bad pixel comes back bit for bit, everything else is finite, the
    result is numpy's, and the pixels no data path connects to the bad one have the clean frame's
    bits."""
    W, H, L, r, f, k = 17, 16, 3, 1, 0, 1.0
    mean, se = pr.odd_frame(W, H, dtype, 5)
    bad = (15, 16) if what == "nan_mean" else (0, 0)
    clean = rt.denoise_pyramid_host(mean, se, None, None, None, pr.SIGMAS, r, f, k, L)
    m, s = mean.copy(), se.copy()
    if what == "nan_mean":
        m[bad][1] = np.nan
    else:
        s[bad] = np.inf
    out = rt.denoise_pyramid_host(m, s, None, None, None, pr.SIGMAS, r, f, k, L)
    dr.check(out, pr.pyramid(m, s, r, f, k, L), f"{what} {np.dtype(dtype).name} vs numpy")
    assert out[bad].tobytes() == m[bad].tobytes()
    others = np.ones((H, W), dtype=bool)
    others[bad] = False
    assert np.isfinite(out[others]).all()
    far = ~_reach((H, W), bad, r, f, L)
    print(f"{what}: {int(far.sum())} of {W * H} pixels out of the bad pixel's reach")
    assert far.sum() >= 40 and not far[bad]
    assert out[far].tobytes() == clean[far].tobytes()
    assert not np.array_equal(out[~far & others], clean[~far & others])


CASES = {"flat": (lambda x: np.full(x.shape, 0.5), 0.05),
         "step": (lambda x: np.where(x < 29, 0.2, 0.8), 0.02),
         "ramp": (lambda x: 0.1 + 0.8 * x / 63.0, 0.03)}


@pytest.mark.parametrize("params", pr.PARAMS, ids=lambda p: "r%d_f%d_k%g" % p)
@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("case", list(CASES))
def test_three_levels_remove_noise_one_level_leaves(rt, case, seed, params):
    """What the filter is for: white noise on a flat field, a step and a ramp (48 x 64 pixels, se the
    luminance's true standard error) has as much power below a small window's cut-off as above it;
    three levels must leave at most 0.9 of one level's RMSE against the truth."""
    truth_fn, sigma = CASES[case]
    x = np.broadcast_to(np.arange(64, dtype=np.float64)[None, :, None], (48, 64, 3))
    truth = truth_fn(x)
    mean = truth + np.random.default_rng(seed).normal(0, sigma, (48, 64, 3))
    se = np.full((48, 64), sigma * np.sqrt(0.2126 ** 2 + 0.7152 ** 2 + 0.0722 ** 2))
    one = dr.rmse(rt.denoise_pyramid_host(mean, se, None, None, None, pr.SIGMAS, *params, 1), truth)
    three = dr.rmse(rt.denoise_pyramid_host(mean, se, None, None, None, pr.SIGMAS, *params, 3), truth)
    print(f"{case} seed {seed} {params}: rmse L=1 {one:.6f}, L=3 {three:.6f}, ratio {three / one:.3f}")
    assert three <= 0.9 * one


def test_ctypes_structs_match_the_c_header(rt, tmp_path):
    """rt_pyramid_params and rt_pyramid_stats: the binding's mirrors have the header's size and
    offsets (compiled with gcc, as tests/test_abi.py checks the older structs)."""
    import os
    import subprocess
    structs = {"rt_pyramid_params": rt.PyramidParams, "rt_pyramid_stats": rt.PyramidStats}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "rt/rt_abi.h"', "int main(void) {"]
    for cname, py in structs.items():
        src.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        src += [f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in py._fields_]
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.run(["gcc", "-I" + inc, str(tmp_path / "layout.c"), "-o", str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout
    for cname, field, val in (line.split() for line in out.splitlines() if line):
        py = structs[cname]
        got = ctypes.sizeof(py) if field == "size" else getattr(py, field).offset
        assert got == int(val), (cname, field, got, int(val))
    assert rt.load_library().rt_abi_version() == 6           # additive: the version stays


def _raw(rt, params, mean, se, guides, out):
    p = lambda x: x.ctypes.data if x is not None else None   # noqa: E731
    return rt.load_library().rt_denoise_pyramid_host(ctypes.byref(params), p(mean), p(se),
                                                     ctypes.byref(guides) if guides is not None else None, p(out))


def test_invalid_arguments(rt):
    W, H = 12, 7
    mean, se, out = np.ones((H, W, 3)), np.zeros((H, W)), np.empty((H, W, 3))
    a, n, z = np.ones((H, W, 3)), np.ones((H, W, 3)), np.ones((H, W))
    par = lambda **kw: rt.PyramidParams(**{**dict(width=W, height=H, format=rt.RT_OUT_F64, on_device=0, radius=3,   # noqa: E731
                                                  patch=1, k=0.45, levels=3, reserved0=0, stream=None), **kw})
    guides = lambda sig=(0.1, 0.2, 0.3), use=(1, 1, 1): rt.DenoiseGuides(   # noqa: E731
        *(g.ctypes.data if u else None for g, u in zip((a, n, z), use)), *sig)
    invalid = lambda rc: rt.ERRORS.get(rc) == "RT_ERR_INVALID" and bool(rt.load_library().rt_last_error())   # noqa: E731
    assert _raw(rt, par(), mean, se, guides(), out) == rt.RT_OK
    assert _raw(rt, par(), mean, se, None, out) == rt.RT_OK
    assert invalid(_raw(rt, par(), mean, se, guides(), mean))                    # out == mean
    assert invalid(_raw(rt, par(), None, se, guides(), out))
    assert invalid(_raw(rt, par(), mean, None, guides(), out))
    assert invalid(_raw(rt, par(), mean, se, guides(), None))
    assert invalid(rt.load_library().rt_denoise_pyramid_host(None, mean.ctypes.data, se.ctypes.data, None, out.ctypes.data))
    for levels in (0, -1, 6):
        assert invalid(_raw(rt, par(levels=levels), mean, se, guides(), out))
    for reserved0 in (1, -1):
        assert invalid(_raw(rt, par(reserved0=reserved0), mean, se, guides(), out))
    for radius in (0, 11):
        assert invalid(_raw(rt, par(radius=radius), mean, se, guides(), out))
    for patch in (-1, 4):
        assert invalid(_raw(rt, par(patch=patch), mean, se, guides(), out))
    for k in (0.0, -1.0, float("nan"), float("inf")):
        assert invalid(_raw(rt, par(k=k), mean, se, guides(), out))
    assert invalid(_raw(rt, par(format=7), mean, se, guides(), out))
    assert invalid(_raw(rt, par(width=0), mean, se, guides(), out))
    assert invalid(_raw(rt, par(height=0), mean, se, guides(), out))
    for v in (0.0, float("nan"), float("inf"), -0.5):
        for i in range(3):
            sig = [0.1, 0.2, 0.3]
            sig[i] = v
            assert invalid(_raw(rt, par(), mean, se, guides(sig), out)), (v, i)
            use = [1, 1, 1]
            use[i] = 0                                       # the sigma of a NULL guide is ignored
            assert _raw(rt, par(), mean, se, guides(sig, use), out) == rt.RT_OK, (v, i)
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
        rt.denoise_pyramid_host(mean, se, levels=6)
    with pytest.raises(rt.RTError):
        rt.denoise_pyramid_host(mean, se, depth=z[:, :5])
