"""rt_denoise_atrous_host: the variance-guided a-trous wavelet filter of include/rt/rt_abi.h on the
host (no device), against the numpy restatement of tests/denoise_atrous_reference.py, under
tests/denoise_reference.py's tolerances (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded
reference in f32). The frames are denoise_reference.cpu_input's (f64 and f32); the guides come from
pixel coordinates (denoise_atrous_reference.coord_guides).
"""
import ctypes

import numpy as np
import pytest

from tests import denoise_atrous_reference as atr
from tests import denoise_reference as dr


def _run(rt, mean, se, levels, variant, guides=None, **kw):
    a, n, z, dem = atr.variant_args(variant, atr.coord_guides(*np.asarray(mean).shape[:2]) if guides is None else guides)
    return rt.denoise_atrous_host(mean, se, a, n, z, atr.SIGMAS, levels, atr.SIGMA_L, dem, **kw)


@pytest.mark.parametrize("variant", atr.VARIANTS)
@pytest.mark.parametrize("levels", atr.LEVELS)
@pytest.mark.parametrize("name", dr.CPU_INPUTS)
def test_host_matches_numpy(rt, name, levels, variant):
    mean, se = dr.cpu_input(name)
    out, se_out = _run(rt, mean, se, levels, variant)
    ref, se_ref = atr.cpu_reference(name, levels, variant)
    assert out.dtype == mean.dtype and np.isfinite(out).all() and np.isfinite(se_out).all()
    what = f"{name} L={levels} {variant}"
    dr.check(out, ref, what + " out")
    dr.check(se_out, se_ref, what + " stderr_out")
    assert not np.array_equal(out, mean)                     # it filters


def test_variants_differ_and_variance_falls(rt):
    """The guides and the demodulation act, and the propagated error is below the input's where
    there was any (every tap weight is positive and sum w^2 V / (sum w)^2 <= max V)."""
    mean, se = dr.cpu_input("random_ragged")
    outs = {v: _run(rt, mean, se, 3, v) for v in atr.VARIANTS}
    assert not np.array_equal(outs["guided"][0], outs["unguided"][0])
    assert not np.array_equal(outs["guided"][0], outs["demodulated"][0])
    se_out = outs["unguided"][1]
    assert se_out.max() <= se.max() * (1 + 1e-12) and se_out.mean() < 0.5 * se.mean()


def test_stderr_out_may_be_null_and_no_guides_is_all_null_guides(rt):
    mean, se = dr.cpu_input("cornell")
    for levels in (1, 5):
        out, se_out = _run(rt, mean, se, levels, "unguided")
        out2, none = _run(rt, mean, se, levels, "unguided", want_stderr=False)
        assert none is None and np.array_equal(out, out2)
        # g == NULL through the raw entry: the bits of all-NULL guides (whose sigmas are ignored)
        m, s = np.ascontiguousarray(mean), np.ascontiguousarray(se)
        raw, raw_se = np.empty_like(m), np.empty_like(s)
        p = rt.AtrousParams(m.shape[1], m.shape[0], rt.RT_OUT_F64, 0, levels, 0, atr.SIGMA_L, None)
        assert rt.load_library().rt_denoise_atrous_host(ctypes.byref(p), m.ctypes.data, s.ctypes.data, None,
                                                        raw.ctypes.data, raw_se.ctypes.data) == rt.RT_OK
        assert np.array_equal(raw, out) and np.array_equal(raw_se, se_out)
        bad_sig, _ = rt.denoise_atrous_host(mean, se, None, None, None, (0.0, float("nan"), -1.0), levels, atr.SIGMA_L)
        assert np.array_equal(bad_sig, out)


@pytest.mark.parametrize("variant", atr.VARIANTS)
def test_non_finite_pixels_stay_and_do_not_spread(rt, variant):
    """A NaN colour channel, an Inf standard error and (demodulated) a NaN albedo: every case matches
    numpy; the NaN-colour and Inf-se pixels come back bit for bit, and nothing else is touched by
    them (no other NaN; the NaN albedo demodulates by 1 and leaves a finite pixel)."""
    mean, se = (np.array(a) for a in dr.cpu_input("random_ragged"))
    guides = [np.array(g) for g in atr.coord_guides(*se.shape)]
    mean[7, 11, 1] = np.nan
    se[15, 30] = np.inf
    if variant == "demodulated":
        guides[0][3, 4, 2] = np.nan
    a, n, z, dem = atr.variant_args(variant, guides)
    for levels in (1, 3, 6):
        out, se_out = rt.denoise_atrous_host(mean, se, a, n, z, atr.SIGMAS, levels, atr.SIGMA_L, dem)
        ref, se_ref = atr.atrous(mean, se, levels, atr.SIGMA_L, a, n, z, atr.SIGMAS, dem)
        dr.check(out, ref, f"non-finite {variant} L={levels} out")
        dr.check(se_out, se_ref, f"non-finite {variant} L={levels} stderr_out")
        assert out[7, 11].tobytes() == mean[7, 11].tobytes() and out[15, 30].tobytes() == mean[15, 30].tobytes()
        assert np.isnan(se_out[7, 11]) == np.isnan(se_ref[7, 11]) and np.isinf(se_out[15, 30])
        nan = np.isnan(out)
        assert nan.sum() == 1 and nan[7, 11, 1]
        assert np.isfinite(out[3, 4]).all() and np.isfinite(np.delete(se_out.reshape(-1), [7 * 37 + 11, 15 * 37 + 30])).all()


def test_ctypes_structs_match_the_c_header(rt, tmp_path):
    """rt_atrous_params and rt_atrous_stats: the binding's mirrors have the header's size and offsets
    (compiled with gcc, as tests/test_abi.py checks the older structs)."""
    import os
    import subprocess
    structs = {"rt_atrous_params": rt.AtrousParams, "rt_atrous_stats": rt.AtrousStats}
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


def _raw(rt, params, mean, se, guides, out, se_out):
    p = lambda x: x.ctypes.data if x is not None else None   # noqa: E731
    return rt.load_library().rt_denoise_atrous_host(ctypes.byref(params), p(mean), p(se),
                                                    ctypes.byref(guides) if guides is not None else None, p(out),
                                                    p(se_out))


def test_invalid_arguments(rt):
    W, H = 12, 7
    mean, se, out, se_out = np.ones((H, W, 3)), np.zeros((H, W)), np.empty((H, W, 3)), np.empty((H, W))
    a, n, z = np.ones((H, W, 3)), np.ones((H, W, 3)), np.ones((H, W))
    par = lambda **kw: rt.AtrousParams(**{**dict(width=W, height=H, format=rt.RT_OUT_F64, on_device=0, levels=3,   # noqa: E731
                                                 demodulate=0, sigma_l=4.0, stream=None), **kw})
    guides = lambda sig=(0.1, 0.2, 0.3), use=(1, 1, 1): rt.DenoiseGuides(   # noqa: E731
        *(g.ctypes.data if u else None for g, u in zip((a, n, z), use)), *sig)
    invalid = lambda rc: rt.ERRORS.get(rc) == "RT_ERR_INVALID" and bool(rt.load_library().rt_last_error())   # noqa: E731
    assert _raw(rt, par(), mean, se, guides(), out, se_out) == rt.RT_OK
    assert _raw(rt, par(demodulate=1), mean, se, guides(), out, None) == rt.RT_OK
    assert invalid(_raw(rt, par(), mean, se, guides(), mean, se_out))            # out == mean
    assert invalid(_raw(rt, par(), mean, se, guides(), out, se))                 # stderr_out == stderr_map
    assert invalid(_raw(rt, par(), None, se, guides(), out, se_out))
    assert invalid(_raw(rt, par(), mean, None, guides(), out, se_out))
    assert invalid(_raw(rt, par(), mean, se, guides(), None, se_out))
    for levels in (0, -1, 7):
        assert invalid(_raw(rt, par(levels=levels), mean, se, guides(), out, se_out))
    for sigma_l in (0.0, -1.0, float("nan"), float("inf")):
        assert invalid(_raw(rt, par(sigma_l=sigma_l), mean, se, guides(), out, se_out))
    for dem in (-1, 2):
        assert invalid(_raw(rt, par(demodulate=dem), mean, se, guides(), out, se_out))
    assert invalid(_raw(rt, par(demodulate=1), mean, se, None, out, se_out))      # demodulate without albedo
    assert invalid(_raw(rt, par(demodulate=1), mean, se, guides(use=(0, 1, 1)), out, se_out))
    assert invalid(_raw(rt, par(format=7), mean, se, guides(), out, se_out))
    assert invalid(_raw(rt, par(width=0), mean, se, guides(), out, se_out))
    for v in (0.0, float("nan"), float("inf"), -0.5):
        for i in range(3):
            sig = [0.1, 0.2, 0.3]
            sig[i] = v
            assert invalid(_raw(rt, par(), mean, se, guides(sig), out, se_out)), (v, i)
            use = [1, 1, 1]
            use[i] = 0                                       # the sigma of a NULL guide is ignored
            assert _raw(rt, par(), mean, se, guides(sig, use), out, se_out) == rt.RT_OK, (v, i)
    with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
        rt.denoise_atrous_host(mean, se, demodulate=True)
    with pytest.raises(rt.RTError):
        rt.denoise_atrous_host(mean, se, depth=z[:, :5])
