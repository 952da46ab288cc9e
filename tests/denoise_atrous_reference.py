"""Reference side of the a-trous denoiser tests (test_denoise_atrous_host.py,
test_denoise_atrous_sanitized.py, test_gpu_denoise_atrous.py): a numpy restatement of the filter
include/rt/rt_abi.h states for rt_denoise_atrous, and deterministic guide frames for the CPU tests,
synthesised from pixel coordinates. Nothing here calls the library under test. Tolerances:
denoise_reference.check's (1e-11 + 1e-11 |ref| in f64, one ulp of the rounded reference in f32).

Why that bound holds over several levels: a perturbation delta of Y changes a weight exp(-dY / dl)
by at most delta / dl * exp(-dY / dl); where dl is at its floor of 1e-10 the weight is already
exp(-dY / 1e-10), and delta / 1e-10 * dY' * exp(-dY' / 1e-10) <= delta / e for the product with
the colour difference the weight multiplies: the error of a level stays of the order of the error
that entered it.
"""
import functools

import numpy as np

from tests import adaptive_reference as ar
from tests import denoise_reference as dr

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)
B3 = (0.25, 0.5, 0.25)
LEVELS = [1, 3, 5, 6]
SIGMA_L = 4.0
SIGMAS = (0.2, 0.3, 0.1)


def albedo_clamp(A):
    """A' of rt_abi.h: the demodulation's divisor."""
    A = np.asarray(A, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(A), np.where(A > 0.01, A, 0.01), 1.0)


def _regions(H, W, oy, ox):
    """The pixels p with p + (ox, oy) inside the image, and their partners; None if there are none."""
    y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def _dist3(F, A, B):
    a = F[A] - F[B]
    return (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]


def _level(C, V, step, sigma_l, guides, inv):
    H, W = V.shape
    Y = ar.luma(C)
    s = np.zeros((H, W))
    ws = np.zeros((H, W))
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            reg = _regions(H, W, dy, dx)
            if reg is None:
                continue
            A, B = reg
            ok = np.isfinite(V[B])
            w = B3[dy + 1] * B3[dx + 1]
            s[A] += np.where(ok, w * V[B], 0.0)
            ws[A] += np.where(ok, w, 0.0)
    vbar = s / ws
    dl = sigma_l * np.sqrt(np.where(vbar > 0.0, vbar, 0.0)) + 1e-10
    num = np.zeros((H, W, 3))
    sw = np.zeros((H, W))
    sv = np.zeros((H, W))
    A_, N_, Z_ = guides
    ia, in_, iz = inv
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            reg = _regions(H, W, step * dy, step * dx)
            if reg is None:
                continue
            A, B = reg
            h = H5[dy + 2] * H5[dx + 2]
            if dx == 0 and dy == 0:
                w = np.full(Y[A].shape, h)
            else:
                e = np.abs(Y[A] - Y[B]) / dl[A]
                if A_ is not None or N_ is not None or Z_ is not None:
                    phi = np.zeros(e.shape)
                    if A_ is not None:
                        phi = phi + _dist3(A_, A, B) * ia
                    if N_ is not None:
                        phi = phi + _dist3(N_, A, B) * in_
                    if Z_ is not None:
                        z = Z_[A] - Z_[B]
                        phi = phi + z * z / (1e-10 + (Z_[A] * Z_[A] + Z_[B] * Z_[B])) * iz
                    e = e + phi
                ok = np.isfinite(e) & np.isfinite(V[B])
                w = np.where(ok, h * np.exp(-e), 0.0)
            take = w != 0.0                                   # w = 0: skipped, not multiplied
            num[A] += np.where(take[..., None], w[..., None] * C[B], 0.0)
            sw[A] += np.where(take, w, 0.0)
            sv[A] += np.where(take, w * w * V[B], 0.0)
    Cn = num / sw[..., None]
    Vn = sv / (sw * sw)
    keep = ~np.isfinite(Y) | ~np.isfinite(V)
    Cn[keep] = C[keep]
    Vn[keep] = V[keep]
    return Cn, Vn


def atrous(mean, se, levels, sigma_l, albedo=None, normal=None, depth=None, sigmas=(1.0, 1.0, 1.0), demodulate=False):
    """The filter of rt_abi.h. mean (H, W, 3) f32 or f64, se (H, W); albedo, normal (H, W, 3) and depth
    (H, W) f64 or None. Returns (out in mean's dtype, stderr_out f64)."""
    M = np.asarray(mean).astype(np.float64)
    se = np.asarray(se, dtype=np.float64)
    guides = tuple(None if g is None else np.asarray(g, dtype=np.float64) for g in (albedo, normal, depth))
    inv = tuple(1.0 / (float(s) * float(s)) for s in sigmas)
    with np.errstate(all="ignore"):
        if demodulate:
            Ap = albedo_clamp(guides[0])
            ya = ar.luma(Ap)
            C = M / Ap
            V = se * se / (ya * ya)
        else:
            C = M.copy()
            V = se * se
        for i in range(levels):
            C, V = _level(C, V, 1 << i, float(sigma_l), guides, inv)
        out = C * Ap if demodulate else C
        se_out = np.sqrt(V * (ya * ya) if demodulate else V)
        keep = ~np.isfinite(ar.luma(M)) | ~np.isfinite(se)
    out[keep] = M[keep]
    return out.astype(np.asarray(mean).dtype), se_out


def coord_guides(H: int, W: int):
    """Guides from pixel coordinates alone: a checker albedo with 5-pixel cells (0.8 / 0.15 tinted),
    a normal that flips across the column W // 3, a depth ramp."""
    y, x = np.mgrid[0:H, 0:W]
    cell = ((x // 5) + (y // 5)) % 2
    albedo = np.where(cell[..., None] == 0, np.array([0.8, 0.7, 0.6]), np.array([0.15, 0.2, 0.25]))
    normal = np.zeros((H, W, 3))
    normal[..., 2] = 1.0
    normal[:, W // 3:] = np.array([1.0, 0.0, 0.0])
    depth = 2.0 + 0.05 * x + 0.02 * y
    return albedo, normal, depth.astype(np.float64)


VARIANTS = ["guided", "unguided", "demodulated"]


def variant_args(variant: str, guides):
    """(albedo, normal, depth, demodulate) of a test variant."""
    if variant == "unguided":
        return None, None, None, False
    return (*guides, variant == "demodulated")


@functools.lru_cache(maxsize=None)
def cpu_reference(name: str, levels: int, variant: str):
    mean, se = dr.cpu_input(name)
    a, n, z, dem = variant_args(variant, coord_guides(*mean.shape[:2]))
    out, se_out = atrous(mean, se, levels, SIGMA_L, a, n, z, SIGMAS, dem)
    out.setflags(write=False)
    se_out.setflags(write=False)
    return out, se_out
