"""Reference side of the denoiser tests (test_denoise_host.py, test_denoise_sanitized.py,
test_gpu_denoise.py): a numpy restatement of the variance-guided NL-means filter that
include/rt/rt_abi.h states for rt_denoise, with direct patch sums (each of the (2f+1)^2 terms added
on its own, no running sums), and the CPU tests' inputs, derived from the CPU oracle. Nothing here
calls the library under test.

Tolerances. f64: 1e-11 + 1e-11 |ref|. Two correct f64 evaluations differed by at most 6e-15 on
these inputs (values up to 15), a running-sum implementation is off by 5e-10 or more: the bound is
~2000 x the first and 50 x below the second. f32 frames: the reference rounded to f32, within one
f32 ulp.
"""
import functools

import numpy as np

from tests import adaptive_reference as ar

TOL_ABS = 1e-11
TOL_REL = 1e-11
PARAMS = [(3, 1, 0.45), (5, 2, 1.0), (10, 3, 0.45), (1, 0, 0.45)]   # (radius, patch, k)


def denoise(mean: np.ndarray, se: np.ndarray, radius: int, patch: int, k: float) -> np.ndarray:
    """The filter of rt_abi.h. mean (H, W, 3) f32 or f64, se (H, W); returns mean's dtype."""
    M = np.asarray(mean).astype(np.float64)
    Y = ar.luma(M)
    V = np.asarray(se, dtype=np.float64) ** 2
    H, W = Y.shape
    r, f = radius, patch
    num = np.zeros((H, W, 3))
    den = np.zeros((H, W))
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                # the pixels a with a and a + o inside the image, and their partners
                y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                A = (slice(y0, y1), slice(x0, x1))
                B = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                h, w_ = y1 - y0, x1 - x0
                if dx == 0 and dy == 0:
                    wgt = np.ones((h, w_))
                else:
                    delta = ((Y[A] - Y[B]) ** 2 - (V[A] + np.minimum(V[A], V[B]))) / (1e-10 + k * k * (V[A] + V[B]))
                    dpad = np.zeros((h + 2 * f, w_ + 2 * f))       # invalid pairs: no term
                    cpad = np.zeros((h + 2 * f, w_ + 2 * f))
                    dpad[f:f + h, f:f + w_] = delta
                    cpad[f:f + h, f:f + w_] = 1.0
                    s = np.zeros((h, w_))
                    c = np.zeros((h, w_))
                    for sy in range(2 * f + 1):
                        for sx in range(2 * f + 1):
                            s = s + dpad[sy:sy + h, sx:sx + w_]
                            c = c + cpad[sy:sy + h, sx:sx + w_]
                    D = s / c
                    wgt = np.where(np.isfinite(D), np.exp(-np.maximum(0.0, D)), 0.0)
                take = wgt != 0.0                                   # w = 0: skipped, not multiplied
                num[A] += np.where(take[..., None], wgt[..., None] * M[B], 0.0)
                den[A] += np.where(take, wgt, 0.0)
        out = num / den[..., None]
    keep = ~np.isfinite(Y) | ~np.isfinite(V)
    out[keep] = M[keep]
    return out.astype(np.asarray(mean).dtype)


def max_excess(got, ref) -> float:
    """max of |got - ref| / (TOL_ABS + TOL_REL |ref|) over finite reference values: <= 1 passes."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - ref[fin]) / (TOL_ABS + TOL_REL * np.abs(ref[fin]))))


def ulps_f32(got, ref) -> int:
    """The largest distance in f32 steps between two finite f32 arrays of the same signs."""
    got, ref = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(ref, dtype=np.float32)
    assert got.shape == ref.shape and np.isfinite(got).all() and np.isfinite(ref).all()
    a, b = got.view(np.int32).astype(np.int64), ref.view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)    # sign-magnitude -> a line
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return int(np.max(np.abs(a - b))) if a.size else 0


def check(got, ref, what: str = "") -> None:
    """got against the reference (of the same dtype): the f64 or the f32 rule above; prints the measured maximum."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape
    if got.dtype == np.float32:
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(got), fin)
        u = ulps_f32(got[fin], ref[fin])
        print(f"{what}: max f32 distance {u} ulp")
        assert u <= 1, what
    else:
        e = max_excess(got, ref)
        print(f"{what}: max |got - ref| / (1e-11 + 1e-11 |ref|) = {e:.3e}")
        assert e <= 1.0, what


def rmse(a, b) -> float:
    return float(np.sqrt(np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)))


def frame_from_samples(samples: np.ndarray, W: int, H: int):
    """(mean, se) of n oracle-derived samples per pixel: the mean frame and the criterion's se."""
    n = samples.shape[0]
    S, Q = ar.moments(samples)
    tile_spp = np.full(((H + 7) // 8, (W + 7) // 8), n, dtype=np.uint32)
    _, _, se = ar.criterion(S, Q, tile_spp, W, H)
    return S / n, se


@functools.lru_cache(maxsize=None)
def cpu_input(name: str):
    """The CPU tests' frames, (mean f64 or f32 (H, W, 3), se (H, W)), read-only."""
    if name == "cornell":
        mean, se = frame_from_samples(ar.oracle_samples(5, 40, 40, 32)[:16], 40, 40)
    elif name == "light":            # 884 of its 960 pixels are black: se = 0
        mean, se = frame_from_samples(ar.oracle_samples(4, 40, 24, 32)[:16], 40, 24)
    elif name == "random_ragged":
        mean, se = frame_from_samples(ar.oracle_samples(0, 37, 21, 32)[:16], 37, 21)
    elif name == "crop":             # 9 x 5: every window of radius 10 is larger than the frame
        m, s = cpu_input("random_ragged")
        mean, se = m[8:13, 14:23].copy(), s[8:13, 14:23].copy()
    elif name == "mixed":            # tiles at 16 and at 32 samples, as test_host_criterion_mixed_counts builds them
        W, H = 40, 24
        samples = ar.oracle_samples(0, W, H, 32)
        tile_spp = np.array([[16, 32, 16, 32, 16], [32, 16, 32, 16, 32], [16, 16, 32, 32, 16]], dtype=np.uint32)
        n_px = ar.tile_map(tile_spp, W, H)
        S16, Q16 = ar.moments(samples[:16])
        S32, Q32 = ar.moments(samples)
        S = np.where((n_px == 16)[..., None], S16, S32)
        Q = np.where(n_px == 16, Q16, Q32)
        _, _, se = ar.criterion(S, Q, tile_spp, W, H)
        mean = S / n_px[..., None]
    elif name == "cornell_f32":
        m, se = cpu_input("cornell")
        mean = m.astype(np.float32)
    else:
        raise KeyError(name)
    mean.setflags(write=False)
    se = np.array(se)
    se.setflags(write=False)
    return mean, se


CPU_INPUTS = ["cornell", "light", "random_ragged", "crop", "mixed", "cornell_f32"]


@functools.lru_cache(maxsize=None)
def cpu_reference(name: str, radius: int, patch: int, k: float) -> np.ndarray:
    out = denoise(*cpu_input(name), radius, patch, k)
    out.setflags(write=False)
    return out
