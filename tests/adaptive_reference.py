"""Reference side of the tile-adaptive sampling tests (test_adaptive_host.py, test_gpu_adaptive.py):
per-sample radiances derived from the CPU oracle, and a numpy restatement of the criterion that
include/rt/rt_abi.h states for rt_render_adaptive. Nothing here calls the library under test.
"""
import functools

import numpy as np

from tests import oracle_binding as ob

TOL_ABS = 1e-6   # on e_px, E_t and se: 100 x the cancellation bound of Q - Ys^2 / n (~1e-8 m, m <= ~15)
TOL_REL = 1e-6


def close(got, ref) -> bool:
    got, ref = np.asarray(got), np.asarray(ref)
    return bool(np.all(np.abs(got - ref) <= TOL_ABS + TOL_REL * np.abs(ref)))


@functools.lru_cache(maxsize=None)
def oracle_samples(scene: int, W: int, H: int, n: int) -> np.ndarray:
    """(n, H, W, 3): sample k of every pixel (scene and render seeds 1 / 1, row 0 = bottom), from the
    oracle's one-chunk means: sample_k = k mean_k - (k - 1) mean_{k-1} (residual <= 4e-15 measured)."""
    out = np.empty((n, H, W, 3), dtype=np.float64)
    prev = np.zeros((H, W, 3), dtype=np.float64)
    for k in range(1, n + 1):
        mean = ob.render(scene, W, H, k, spp_chunk=1 << 20)
        out[k - 1] = k * mean - (k - 1) * prev
        prev = mean
    out.setflags(write=False)
    return out


def luma(c: np.ndarray) -> np.ndarray:
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def moments(samples: np.ndarray):
    """S (H, W, 3) and Q (H, W) of the given samples."""
    return samples.sum(axis=0), (luma(samples) ** 2).sum(axis=0)


def tile_map(values: np.ndarray, W: int, H: int) -> np.ndarray:
    """A (tiles_y, tiles_x) array spread to (H, W): each pixel its tile's value."""
    return np.repeat(np.repeat(values, 8, axis=0), 8, axis=1)[:H, :W]


def criterion(S: np.ndarray, Q: np.ndarray, tile_spp: np.ndarray, W: int, H: int):
    """The criterion of rt_abi.h: (e_px (H, W), E_t (tiles_y, tiles_x), se (H, W))."""
    ty, tx = (H + 7) // 8, (W + 7) // 8
    n = tile_map(np.asarray(tile_spp, dtype=np.float64).reshape(ty, tx), W, H)
    ys = luma(S)
    m = ys / n
    var = np.maximum(0.0, (Q - ys * ys / n) / (n - 1.0))
    se = np.sqrt(var / n)
    e = se / np.sqrt(np.maximum(m, 1e-4))
    E = np.empty((ty, tx), dtype=np.float64)
    for j in range(ty):
        for i in range(tx):
            E[j, i] = e[8 * j:8 * j + 8, 8 * i:8 * i + 8].mean()   # in-image pixels only: e is (H, W)
    return e, E, se


def simulate(samples: np.ndarray, W: int, H: int, spp: int, min_spp: int, step_spp: int, threshold: float):
    """The stop rule on reference samples (min_spp and step_spp already multiples of the chunk).
    Returns (tile_spp (tiles_y, tiles_x), S, Q at each tile's own count, E_t at each tile's last
    pass, se, and `tested`: every E_t the rule compared with the threshold, at any pass)."""
    ty, tx = (H + 7) // 8, (W + 7) // 8
    tile_spp = np.zeros((ty, tx), dtype=np.int64)
    active = np.ones((ty, tx), dtype=bool)
    S = np.zeros((H, W, 3))
    Q = np.zeros((H, W))
    E_last = np.zeros((ty, tx))
    tested = []
    done = 0
    while active.any() and done < spp:
        end = min(spp, done + (min_spp if done == 0 else step_spp))
        Sn, Qn = moments(samples[:end])
        _, E, _ = criterion(Sn, Qn, np.full((ty, tx), end), W, H)
        tested.extend(E[active].tolist())
        px = tile_map(active, W, H)
        S[px], Q[px] = Sn[px], Qn[px]
        tile_spp[active] = end
        E_last[active] = E[active]
        stop = active & ((E <= threshold) if threshold > 0 else np.zeros_like(active)) | (active & (end >= spp))
        active &= ~stop
        done = end
    _, _, se = criterion(S, Q, tile_spp, W, H)
    return tile_spp, S, Q, E_last, se, np.array(tested)
