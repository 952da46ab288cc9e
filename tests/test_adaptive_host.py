"""rt_adaptive_tile_errors_host: the adaptive-sampling criterion of include/rt/rt_abi.h on the host
(no device), against a numpy restatement on per-sample radiances derived from the CPU oracle.

Tolerance on e_px / se and E_t: 1e-6 absolute plus 1e-6 relative. The cancellation in
Q - Ys^2 / n bounds the difference two correct f64 evaluations can show at about
sqrt(2^-53 m^2 / (n - 1)) ~ 1e-8 m, 100 x smaller even at the Cornell light's m ~ 15.
"""
import numpy as np
import pytest

from tests import adaptive_reference as ar


def _reference(scene, W, H, n):
    samples = ar.oracle_samples(scene, W, H, 32)[:n]
    S, Q = ar.moments(samples)
    ty, tx = (H + 7) // 8, (W + 7) // 8
    tile_spp = np.full((ty, tx), n, dtype=np.uint32)
    return samples, S, Q, tile_spp


@pytest.mark.parametrize("scene,W,H,n", [(0, 40, 24, 16), (0, 40, 24, 32), (0, 36, 20, 16), (4, 40, 24, 16)])
def test_host_criterion_matches_numpy(rt, scene, W, H, n):
    """Whole tiles (40x24), ragged tiles (36x20: only the in-image pixels count) and the light
    scene, whose all-black tiles give e_px = 0 exactly (no division by zero)."""
    samples, S, Q, tile_spp = _reference(scene, W, H, n)
    e_ref, E_ref, se_ref = ar.criterion(S, Q, tile_spp, W, H)
    E, se = rt.adaptive_tile_errors_host(S, Q, tile_spp, W, H)
    E = E.reshape(E_ref.shape)
    assert np.isfinite(E).all() and np.isfinite(se).all()
    print(f"max |E - ref| = {np.abs(E - E_ref).max():.3e}, max |se - ref| = {np.abs(se - se_ref).max():.3e}")
    assert ar.close(E, E_ref)
    assert ar.close(se, se_ref)
    m = np.maximum(ar.luma(S) / n, 1e-4)
    assert ar.close(se / np.sqrt(m), e_ref)          # e_px from the library's se
    assert (E >= 0).all() and E.max() > 0.01
    if scene == 4:
        black = np.array([[not samples[:, 8 * j:8 * j + 8, 8 * i:8 * i + 8].any() for i in range(E.shape[1])]
                          for j in range(E.shape[0])])
        assert black.any() and not black.all()
        assert (E[black] == 0.0).all() and (E[~black] > 0).all()
        assert (se[ar.tile_map(black, W, H)] == 0.0).all()


def test_host_criterion_mixed_counts(rt):
    """Tiles at different sample counts, as an adaptive frame leaves them."""
    W, H = 40, 24
    samples = ar.oracle_samples(0, W, H, 32)
    tile_spp = np.array([[16, 32, 16, 32, 16], [32, 16, 32, 16, 32], [16, 16, 32, 32, 16]], dtype=np.uint32)
    n_px = ar.tile_map(tile_spp, W, H)
    S16, Q16 = ar.moments(samples[:16])
    S32, Q32 = ar.moments(samples)
    S = np.where((n_px == 16)[..., None], S16, S32)
    Q = np.where(n_px == 16, Q16, Q32)
    _, E_ref, se_ref = ar.criterion(S, Q, tile_spp, W, H)
    E, se = rt.adaptive_tile_errors_host(S, Q, tile_spp, W, H)
    assert ar.close(E.reshape(E_ref.shape), E_ref) and ar.close(se, se_ref)


def test_host_criterion_needs_two_samples(rt):
    """A tile with n < 2 has no variance estimate: RT_ERR_INVALID."""
    W, H = 16, 8
    S, Q = np.ones((H, W, 3)), np.ones((H, W))
    for bad in ([1, 4], [4, 0]):
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID"):
            rt.adaptive_tile_errors_host(S, Q, np.array(bad, dtype=np.uint32), W, H)
    rt.adaptive_tile_errors_host(S, Q, np.array([2, 2], dtype=np.uint32), W, H)
