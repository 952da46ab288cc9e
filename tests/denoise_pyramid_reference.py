"""Reference side of the pyramid-denoiser tests (test_denoise_pyramid_host.py,
test_denoise_pyramid_sanitized.py, test_gpu_denoise_pyramid.py): a numpy restatement of the filter
include/rt/rt_abi.h states for rt_denoise_pyramid, around tests/denoise_guided_reference.py's filter
per level. Nothing here calls the library under test. Tolerances: denoise_reference.check's
(1e-11 + 1e-11 |ref| in f64, one ulp of the rounded reference in f32).

Why that bound holds over several levels: Down, the block means of Up and the four-tap correction
are a handful of f64 operations in a stated order, which numpy and the library do alike, so every
level's input is the same bits on both sides; what differs is each level's filter, by its exp
(6e-15 measured between two correct evaluations, denoise_reference.py), and R_0 adds at most L such
errors with weights that sum to 1 per level.
"""
import functools

import numpy as np

from tests import adaptive_reference as ar
from tests import denoise_atrous_reference as atr
from tests import denoise_guided_reference as gr
from tests import denoise_reference as dr

LEVELS = [1, 2, 3, 5]
PARAMS = [(3, 1, 0.45), (5, 2, 1.0)]           # (radius, patch, k)
SIGMAS = gr.SIGMAS
ODD_SIZES = [(1, 1), (2, 1), (3, 3), (9, 5), (72, 9)]   # (W, H): blocks of 1 and 2 pixels, clamped taps on both axes
TAPS = (9.0 / 16.0, 3.0 / 16.0, 3.0 / 16.0, 1.0 / 16.0)


def _block_terms(F):
    """The up to four terms of every block of F (H, W[, ch]) in raster order, as (term padded to the
    coarse grid, its inside mask (hc, wc)) pairs, and n (hc, wc)."""
    H, W = F.shape[:2]
    hc, wc = (H + 1) // 2, (W + 1) // 2
    terms = []
    n = np.zeros((hc, wc))
    for j in (0, 1):
        for i in (0, 1):
            sub = F[j::2, i::2]
            inside = np.zeros((hc, wc), dtype=bool)
            inside[:sub.shape[0], :sub.shape[1]] = True
            full = np.zeros((hc, wc) + F.shape[2:])
            full[:sub.shape[0], :sub.shape[1]] = sub
            terms.append((full, inside))
            n += inside
    return terms, n


def block_mean(F):
    """The Down rule for a colour or guide frame: the raster-order sum from 0.0 over the block, / n."""
    terms, n = _block_terms(F)
    s = np.zeros(terms[0][0].shape)
    for full, inside in terms:
        m = inside if full.ndim == 2 else inside[..., None]
        s = np.where(m, s + full, s)
    return s / (n if s.ndim == 2 else n[..., None])


def block_se(S):
    """s_{l+1} = sqrt(sum s s) / n."""
    terms, n = _block_terms(S)
    t = np.zeros(n.shape)
    for full, inside in terms:
        t = np.where(inside, t + full * full, t)
    return np.sqrt(t) / n


def tap_coords(n, nc):
    """(c, o) of the contract for the fine coordinates 0..n-1 against a coarse axis of nc."""
    x = np.arange(n)
    c = x // 2
    o = np.clip(np.where(x % 2 == 0, c - 1, c + 1), 0, nc - 1)
    return c, o


def correction(K, H, W):
    """u (H, W, 3) from K (hc, wc, 3)."""
    hc, wc = K.shape[:2]
    cx, ox = tap_coords(W, wc)
    cy, oy = tap_coords(H, hc)
    ok = np.isfinite(K).all(axis=2)
    num = np.zeros((H, W, 3))
    sw = np.zeros((H, W))
    for wgt, (ty, tx) in zip(TAPS, ((cy, cx), (cy, ox), (oy, cx), (oy, ox))):
        k = K[ty[:, None], tx[None, :]]
        take = ok[ty[:, None], tx[None, :]]
        num = np.where(take[..., None], num + wgt * k, num)
        sw = np.where(take, sw + wgt, sw)
    return np.where((sw > 0.0)[..., None], num / np.where(sw > 0.0, sw, 1.0)[..., None], 0.0)


def pyramid(mean, se, radius, patch, k, levels, albedo=None, normal=None, depth=None, sigmas=(1.0, 1.0, 1.0)):
    """The filter of rt_abi.h. mean (H, W, 3) f32 or f64, se (H, W); albedo, normal (H, W, 3) and depth
    (H, W) f64 or None. Returns mean's dtype."""
    M = np.asarray(mean).astype(np.float64)
    se = np.asarray(se, dtype=np.float64)
    C, S = [M], [se]
    G = [tuple(None if g is None else np.asarray(g, dtype=np.float64) for g in (albedo, normal, depth))]
    with np.errstate(all="ignore"):
        for _ in range(levels - 1):
            C.append(block_mean(C[-1]))
            S.append(block_se(S[-1]))
            G.append(tuple(None if g is None else block_mean(g) for g in G[-1]))
        D = [gr.denoise_guided(C[l], S[l], radius, patch, k, *G[l], sigmas) for l in range(levels)]
        R = D[levels - 1]
        for l in range(levels - 2, -1, -1):
            K = R - block_mean(D[l])
            R = D[l] + correction(K, *D[l].shape[:2])
        keep = ~np.isfinite(ar.luma(M)) | ~np.isfinite(se)
    out = np.array(R)
    out[keep] = M[keep]
    return out.astype(np.asarray(mean).dtype)


def odd_frame(W, H, dtype=np.float64, seed=0):
    """A frame of an odd size: test_denoise_sanitized's ramp plus stated noise."""
    from tests.test_denoise_sanitized import _frame
    return _frame(W, H, dtype, 71 + seed)


def guides_for(mean, guided: bool):
    return atr.coord_guides(*np.asarray(mean).shape[:2]) if guided else (None, None, None)


@functools.lru_cache(maxsize=None)
def cpu_frame(name):
    """A CPU test frame by name: denoise_reference.cpu_input's, or 'WxH' / 'WxH_f32' for an odd size."""
    if name in dr.CPU_INPUTS:
        return dr.cpu_input(name)
    size, _, fmt = name.partition("_")
    W, H = (int(v) for v in size.split("x"))
    mean, se = odd_frame(W, H, np.float32 if fmt == "f32" else np.float64, W + H)
    mean.setflags(write=False)
    se.setflags(write=False)
    return mean, se


CPU_FRAMES = list(dr.CPU_INPUTS) + [f"{W}x{H}{sfx}" for W, H in ODD_SIZES for sfx in ("", "_f32")]


@functools.lru_cache(maxsize=None)
def cpu_reference(name: str, radius: int, patch: int, k: float, levels: int, guided: bool):
    mean, se = cpu_frame(name)
    out = pyramid(mean, se, radius, patch, k, levels, *guides_for(mean, guided), SIGMAS)
    out.setflags(write=False)
    return out
