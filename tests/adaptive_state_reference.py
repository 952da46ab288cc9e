"""Reference side of the rt_adaptive_state tests (test_adaptive_state_host.py,
test_gpu_adaptive_state.py): the selection rule and the advance loop that include/rt/rt_abi.h states,
restated in numpy over adaptive_reference's moments and criterion on oracle-derived samples.
Nothing here calls the library under test.
"""
import numpy as np

from tests import adaptive_reference as ar


def next_count(n: int, cap: int, min_r: int, step_r: int) -> int:
    return min(cap, min_r if n == 0 else n + step_r)


def stops(E, threshold: float):
    """rt_render_adaptive's predicate: a threshold <= 0 stops nothing, nor does a NaN error."""
    E = np.asarray(E, dtype=np.float64)
    if not threshold > 0:
        return np.zeros(E.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        return E <= threshold


def active(tile_spp, E, threshold: float, cap: int):
    n = np.asarray(tile_spp).astype(np.int64)
    return (n < cap) & ((n == 0) | ~stops(E, threshold))


def next_group(tile_spp, threshold, cap, min_r, step_r, tile_error=None, selected=None):
    """(group: flat raster indices ascending, n_star, n_next, n_active); no active tile: ([], 0, 0, 0)."""
    n = np.asarray(tile_spp).astype(np.int64).reshape(-1)
    if selected is not None:
        act = (np.asarray(selected).reshape(-1) != 0) & (n < cap)
    else:
        act = active(n, np.asarray(tile_error, dtype=np.float64).reshape(-1), threshold, cap)
    if not act.any():
        return np.zeros(0, dtype=np.int64), 0, 0, 0
    n_star = int(n[act].min())
    return np.flatnonzero(act & (n == n_star)), n_star, next_count(n_star, cap, min_r, step_r), int(act.sum())


class SimState:
    """The state of rt_abi.h on reference samples (n_max, H, W, 3): every tile at its own count, its
    E_t from the numpy criterion at that count. `tested` collects every E_t a call compared with its
    threshold, for the margin the GPU tests assert."""

    def __init__(self, samples: np.ndarray, W: int, H: int, min_r: int, step_r: int):
        self.samples, self.W, self.H, self.min_r, self.step_r = samples, W, H, min_r, step_r
        self.ty, self.tx = (H + 7) // 8, (W + 7) // 8
        self.tile_spp = np.zeros((self.ty, self.tx), dtype=np.int64)
        self.E = np.zeros((self.ty, self.tx))
        self.groups = self.samples_traced = 0          # of the last advance
        self.groups_total = self.samples_total = 0
        self.tested = []
        self._E_at = {}

    def E_at(self, n: int) -> np.ndarray:
        if n not in self._E_at:
            S, Q = ar.moments(self.samples[:n])
            self._E_at[n] = ar.criterion(S, Q, np.full((self.ty, self.tx), n), self.W, self.H)[1]
        return self._E_at[n]

    def _step(self, group: np.ndarray, n_star: int, n_next: int):
        flat_n, flat_E = self.tile_spp.reshape(-1), self.E.reshape(-1)
        flat_n[group] = n_next
        flat_E[group] = self.E_at(n_next).reshape(-1)[group]
        self.groups += 1
        self.samples_traced += 64 * group.size * (n_next - n_star)

    def advance(self, threshold: float, cap: int, max_launches: int = 0, tile_error_in=None) -> int:
        self.groups = self.samples_traced = 0
        sel = None
        if tile_error_in is not None:   # one round: the set is fixed here, every member stepped once
            sel = (~stops(np.asarray(tile_error_in).reshape(-1), threshold)) & (self.tile_spp.reshape(-1) < cap)
        while True:
            if sel is None:
                seen = (self.tile_spp > 0) & (self.tile_spp < cap)
                if threshold > 0:
                    self.tested.extend((self.E[seen] / threshold).tolist())
            g, n_star, n_next, n_active = next_group(self.tile_spp, threshold, cap, self.min_r, self.step_r,
                                                     tile_error=self.E if sel is None else None, selected=sel)
            if g.size == 0 or (max_launches and self.groups >= max_launches):
                break
            self._step(g, n_star, n_next)
            if sel is not None:
                sel[g] = False
        self.groups_total += self.groups
        self.samples_total += self.samples_traced
        return n_active

    def margin(self) -> float:
        """The smallest relative distance of a compared E_t from its threshold so far."""
        t = np.asarray(self.tested)
        t = t[np.isfinite(t)]
        return float(np.min(np.abs(t - 1.0))) if t.size else float("inf")

    def frame(self):
        """(S, Q, se) with every tile at its own count."""
        n_px = ar.tile_map(self.tile_spp, self.W, self.H)
        S, Q = np.zeros((self.H, self.W, 3)), np.zeros((self.H, self.W))
        for n in sorted(set(self.tile_spp.reshape(-1).tolist())):
            Sn, Qn = ar.moments(self.samples[:n])
            S[n_px == n], Q[n_px == n] = Sn[n_px == n], Qn[n_px == n]
        return S, Q, ar.criterion(S, Q, self.tile_spp, self.W, self.H)[2]
