"""Reference side of the cross-filter tests (test_denoise_cross_host.py,
test_denoise_cross_sanitized.py, test_gpu_denoise_cross.py): a numpy restatement of the filter that
include/rt/rt_abi.h states for rt_denoise_cross, with direct patch sums (each of the (2f+1)^2 terms
added on its own), and the CPU tests' half frames, derived from the CPU oracle's samples by parity.
Nothing here calls the library under test. Tolerances: denoise_reference.check's (1e-11 + 1e-11 |ref|
in f64, one f32 ulp), for out and for stderr_out.
"""
import functools

import numpy as np

from tests import adaptive_reference as ar
from tests import denoise_reference as dr


def _dist3(F, A, B):
    a = F[A] - F[B]
    return (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]


def stderr_from_e(e: np.ndarray) -> np.ndarray:
    """stderr_out from e: sqrt of the 3 x 3 binomial mean of E2 = e e over the neighbours inside the
    image with a finite E2, divided by the weights taken, in raster order; sqrt(E2(p)) where E2(p)
    is not finite."""
    H, W = e.shape
    with np.errstate(all="ignore"):
        E2 = e * e
        s = np.zeros((H, W))
        ws = np.zeros((H, W))
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                A = (slice(y0, y1), slice(x0, x1))
                B = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                w = (0.5 if dy == 0 else 0.25) * (0.5 if dx == 0 else 0.25)
                v = E2[B]
                ok = np.isfinite(v)
                s[A] += np.where(ok, w * v, 0.0)
                ws[A] += np.where(ok, w, 0.0)
        out = np.sqrt(s / ws)
        bad = ~np.isfinite(E2)
        out[bad] = np.sqrt(E2[bad])
    return out


def denoise_cross(mean_a, mean_b, se, radius, patch, k, scale, albedo=None, normal=None, depth=None,
                  sigmas=(1.0, 1.0, 1.0)):
    """The filter of rt_abi.h. mean_a, mean_b (H, W, 3) f32 or f64, se (H, W); the guides (H, W, 3),
    (H, W, 3), (H, W) f64 or None. Returns (out in the means' dtype, stderr_out (H, W) f64)."""
    MA = np.asarray(mean_a).astype(np.float64)
    MB = np.asarray(mean_b).astype(np.float64)
    with np.errstate(all="ignore"):
        YA, YB = ar.luma(MA), ar.luma(MB)
        s_ = np.asarray(se, dtype=np.float64)
        V = scale * (s_ * s_)
    bad = ~np.isfinite(YA) | ~np.isfinite(YB) | ~np.isfinite(V)
    YA = np.where(bad, np.nan, YA)
    YB = np.where(bad, np.nan, YB)
    H, W = YA.shape
    r, f = radius, patch
    A_, N_, Z_ = (None if g is None else np.asarray(g, dtype=np.float64) for g in (albedo, normal, depth))
    ia, in_, iz = (1.0 / (float(s) * float(s)) for s in sigmas)
    num_a, num_b = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    den_a, den_b = np.zeros((H, W)), np.zeros((H, W))
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
                if y0 >= y1 or x0 >= x1:
                    continue
                A = (slice(y0, y1), slice(x0, x1))
                B = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                h, w_ = y1 - y0, x1 - x0
                if dx == 0 and dy == 0:
                    wa = wb = np.ones((h, w_))
                else:
                    cpad = np.zeros((h + 2 * f, w_ + 2 * f))
                    cpad[f:f + h, f:f + w_] = 1.0
                    c = np.zeros((h, w_))
                    for sy in range(2 * f + 1):
                        for sx in range(2 * f + 1):
                            c = c + cpad[sy:sy + h, sx:sx + w_]
                    phi = np.zeros((h, w_))                        # per pixel pair, left to right
                    if A_ is not None:
                        phi = phi + _dist3(A_, A, B) * ia
                    if N_ is not None:
                        phi = phi + _dist3(N_, A, B) * in_
                    if Z_ is not None:
                        z = Z_[A] - Z_[B]
                        phi = phi + z * z / (1e-10 + (Z_[A] * Z_[A] + Z_[B] * Z_[B])) * iz
                    w = []
                    for Y in (YA, YB):
                        delta = ((Y[A] - Y[B]) ** 2 - (V[A] + np.minimum(V[A], V[B]))) / (1e-10 + k * k * (V[A] + V[B]))
                        dpad = np.zeros((h + 2 * f, w_ + 2 * f))   # invalid pairs: no term
                        dpad[f:f + h, f:f + w_] = delta
                        s = np.zeros((h, w_))
                        for sy in range(2 * f + 1):
                            for sx in range(2 * f + 1):
                                s = s + dpad[sy:sy + h, sx:sx + w_]
                        D = s / c
                        ok = np.isfinite(D) & np.isfinite(phi)
                        w.append(np.where(ok, np.exp(-(np.maximum(0.0, D) + phi)), 0.0))
                    wa, wb = w
                # cross application; w = 0: skipped, not multiplied
                ta, tb = wb != 0.0, wa != 0.0
                num_a[A] += np.where(ta[..., None], wb[..., None] * MA[B], 0.0)
                den_a[A] += np.where(ta, wb, 0.0)
                num_b[A] += np.where(tb[..., None], wa[..., None] * MB[B], 0.0)
                den_b[A] += np.where(tb, wa, 0.0)
        FA = num_a / den_a[..., None]
        FB = num_b / den_b[..., None]
        FA[bad] = MA[bad]
        FB[bad] = MB[bad]
        out = 0.5 * (FA + FB)
        e = 0.5 * (ar.luma(FA) - ar.luma(FB))
    return out.astype(np.asarray(mean_a).dtype), stderr_from_e(e)


SCALE = 2.0


def _halves(samples: np.ndarray, n_px: np.ndarray):
    """The half means of a frame whose pixel (y, x) took its first n_px[y, x] samples: A the even
    sample indices, B the odd ones."""
    H, W = n_px.shape
    A, B = np.empty((H, W, 3)), np.empty((H, W, 3))
    for n in np.unique(n_px):
        m = n_px == n
        A[m] = samples[:n][0::2].mean(axis=0)[m]
        B[m] = samples[:n][1::2].mean(axis=0)[m]
    return A, B


@functools.lru_cache(maxsize=None)
def cpu_input(name: str):
    """The CPU tests' frames, (mean_a, mean_b, se), read-only: denoise_reference.cpu_input's frames
    with their samples split by parity; se is that frame's (the whole mean's)."""
    _, se = dr.cpu_input(name)
    if name == "cornell":
        a, b = _halves(ar.oracle_samples(5, 40, 40, 32), np.full((40, 40), 16))
    elif name == "light":
        a, b = _halves(ar.oracle_samples(4, 40, 24, 32), np.full((24, 40), 16))
    elif name == "random_ragged":
        a, b = _halves(ar.oracle_samples(0, 37, 21, 32), np.full((21, 37), 16))
    elif name == "crop":
        ra, rb, _ = cpu_input("random_ragged")
        a, b = ra[8:13, 14:23].copy(), rb[8:13, 14:23].copy()
    elif name == "mixed":
        tile_spp = np.array([[16, 32, 16, 32, 16], [32, 16, 32, 16, 32], [16, 16, 32, 32, 16]], dtype=np.uint32)
        a, b = _halves(ar.oracle_samples(0, 40, 24, 32), ar.tile_map(tile_spp, 40, 24).astype(np.int64))
    elif name == "cornell_f32":
        a, b, _ = cpu_input("cornell")
        a, b = a.astype(np.float32), b.astype(np.float32)
    else:
        raise KeyError(name)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, se


@functools.lru_cache(maxsize=None)
def cpu_reference(name: str, radius: int, patch: int, k: float, guided: bool):
    """(out, stderr_out) of the reference on cpu_input(name) at scale 2, read-only; guided: with
    denoise_guided_reference.cpu_guides of the whole mean and its SIGMAS."""
    from tests import denoise_guided_reference as gr
    a, b, se = cpu_input(name)
    kw = {}
    if guided:
        al, no, de = gr.cpu_guides(dr.cpu_input(name)[0])
        kw = dict(albedo=al, normal=no, depth=de, sigmas=gr.SIGMAS)
    out, so = denoise_cross(a, b, se, radius, patch, k, SCALE, **kw)
    out.setflags(write=False)
    so.setflags(write=False)
    return out, so
