"""Reference side of the guided-denoiser tests (test_denoise_guided_host.py,
test_denoise_guided_sanitized.py, test_gpu_denoise_guided.py): a numpy restatement of the filter
include/rt/rt_abi.h states for rt_denoise_guided — tests/denoise_reference.py's denoise() with the
feature term Phi in the weight — and deterministic guide frames for the CPU tests. Nothing here
calls the library under test. Tolerances: denoise_reference.check's.
"""
import numpy as np

from tests import adaptive_reference as ar


def _dist3(F, A, B):
    a = F[A] - F[B]
    return (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]


def denoise_guided(mean, se, radius, patch, k, albedo=None, normal=None, depth=None, sigmas=(1.0, 1.0, 1.0)):
    """The guided filter of rt_abi.h. mean (H, W, 3) f32 or f64, se (H, W); albedo, normal (H, W, 3)
    and depth (H, W) f64 or None; sigmas = (albedo, normal, depth). Returns mean's dtype."""
    M = np.asarray(mean).astype(np.float64)
    Y = ar.luma(M)
    V = np.asarray(se, dtype=np.float64) ** 2
    H, W = Y.shape
    r, f = radius, patch
    A_, N_, Z_ = (None if g is None else np.asarray(g, dtype=np.float64) for g in (albedo, normal, depth))
    ia, in_, iz = (1.0 / (float(s) * float(s)) for s in sigmas)
    num = np.zeros((H, W, 3))
    den = np.zeros((H, W))
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
                    phi = np.zeros((h, w_))                        # per pixel pair, left to right
                    if A_ is not None:
                        phi = phi + _dist3(A_, A, B) * ia
                    if N_ is not None:
                        phi = phi + _dist3(N_, A, B) * in_
                    if Z_ is not None:
                        z = Z_[A] - Z_[B]
                        phi = phi + z * z / (1e-10 + (Z_[A] * Z_[A] + Z_[B] * Z_[B])) * iz
                    ok = np.isfinite(D) & np.isfinite(phi)
                    wgt = np.where(ok, np.exp(-(np.maximum(0.0, D) + phi)), 0.0)
                take = wgt != 0.0                                   # w = 0: skipped, not multiplied
                num[A] += np.where(take[..., None], wgt[..., None] * M[B], 0.0)
                den[A] += np.where(take, wgt, 0.0)
        out = num / den[..., None]
    keep = ~np.isfinite(Y) | ~np.isfinite(V)
    out[keep] = M[keep]
    return out.astype(np.asarray(mean).dtype)


SIGMAS = (0.2, 0.3, 0.1)


def cpu_guides(mean, seed: int = 5):
    """Deterministic guides for a CPU frame: albedo = the frame clipped to [0, 1]; normal and depth
    from a fixed-seed generator, quantised to a few levels (so neighbours share values and the
    feature term is 0 for some pairs and large for others)."""
    m = np.asarray(mean, dtype=np.float64)
    H, W = m.shape[:2]
    rng = np.random.default_rng(seed)
    albedo = np.clip(m, 0.0, 1.0)
    normal = np.round(rng.uniform(-1.0, 1.0, (H, W, 3)) * 2.0) / 2.0      # 5 levels per component
    depth = 1.0 + np.round(rng.uniform(0.0, 1.0, (H, W)) * 3.0)           # 1, 2, 3, 4
    return albedo, normal, depth
