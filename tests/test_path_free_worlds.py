"""The reference alone meets every condition tests/test_gpu_f32_exact.py relies on (CPU).

The path-independent worlds of tests/path_free_worlds.py, rendered by the oracle at four
render seeds: the one-bounce lattice holds exactly, the furnace's black samples stay two
orders below the GPU test's cap, the ID worlds have the interior pixels the GPU test
compares, and the noise emitter's second seed lies inside the first seed's bracket. A GPU
test failing on these worlds can then only be the kernel.
"""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import path_free_worlds as pf

ONE_BOUNCE = pf.one_bounce_worlds()
ID_WORLDS = pf.id_worlds()


def _oracle_renders(spec, seeds=pf.SEEDS):
    w = ob.OracleWorld(1)
    try:
        spec.build(w)
        return [w.render(spec.cam24(), pf.BG, spec.W, spec.H, spec.spp, render_seed=s) for s in seeds]
    finally:
        w.close()


def test_camera24_is_the_reference_camera():
    """The numpy camera against the oracle's own for a preset scene (scene 0: look_from
    (13, 2, 3), vfov 20; its aperture and focus distance passed through)."""
    ref = ob.camera(0, 48, 32)
    got = pf.camera24((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, 48 / 32, aperture=2.0 * ref[21], focus_dist=10.0)
    assert np.allclose(got, ref, rtol=0, atol=1e-12), np.abs(got - ref).max()


@pytest.mark.parametrize("spec", ONE_BOUNCE, ids=[s.name for s in ONE_BOUNCE])
def test_one_bounce_worlds_sit_on_the_lattice(spec):
    for seed, img in zip(pf.SEEDS, _oracle_renders(spec)):
        ok, j = pf.lattice_j(img, pf.BG, spec.albedo, spec.spp, 1e-9)
        assert ok.all(), f"{spec.name} seed {seed}: {int((~ok).sum())} off-lattice pixels"
        if spec.albedo is not None:
            hit = j.sum() / (spec.W * spec.H * spec.spp)
            assert 0.05 <= hit <= 0.95, f"{spec.name} seed {seed}: hit share {hit}"


@pytest.mark.parametrize("full", [True, False], ids=["full", "media"])
def test_furnace_is_bg_or_black(full):
    spec = pf.furnace_world(full)
    for seed, img in zip(pf.SEEDS, _oracle_renders(spec)):
        ok, n_black = pf.furnace_black(img, pf.BG, spec.spp, 1e-9)
        assert ok.all(), f"{spec.name} seed {seed}: {int((~ok).sum())} pixels off the black-sample lattice"
        share = n_black / (spec.W * spec.H * spec.spp)
        assert share <= 1e-4, f"{spec.name} seed {seed}: black share {share}"
        assert float(img.max()) <= 1.0 + 1e-12


@pytest.mark.parametrize("spec", ID_WORLDS, ids=[s.name for s in ID_WORLDS])
def test_id_worlds_have_interior_pixels_of_every_class(spec):
    imgs = _oracle_renders(spec)
    inner = pf.interior(imgs)
    share = float(inner.mean())
    assert share >= spec.min_share, f"{spec.name}: interior share {share}"
    for im in imgs[1:]:
        assert np.array_equal(im[inner], imgs[0][inner]), spec.name     # bit-equal across the seeds
    # every interior pixel is a palette colour or the background
    known = np.all(np.abs(imgs[0] - np.asarray(pf.BG)) <= 1e-12, axis=-1)
    for c, _ in spec.owners:
        known |= np.all(np.abs(imgs[0] - np.asarray(c)) <= 1e-12, axis=-1)
    assert known[inner].all(), spec.name
    cols = np.array([c for c, _ in spec.owners] + [pf.BG])
    d = np.abs(cols[:, None, :] - cols[None, :, :]).max(axis=-1) + np.eye(len(cols))
    assert d.min() >= 0.05 - 1e-12, (spec.name, d.min())
    if spec.n_spheres:      # the big field's looser condition
        assert len(spec.owners) == spec.n_spheres > 1023
        assert pf.colours_owning(imgs[0], inner, spec.owners) >= spec.n_spheres // 2
    else:
        counts = pf.owner_counts(imgs[0], inner, spec.owners)
        assert all(n >= 20 for n in counts.values()), (spec.name, counts)


def test_noise_emitter_second_seed_lies_in_the_first_seeds_bracket():
    spec = pf.noise_world()
    imgs = _oracle_renders(spec)
    on_sphere = pf.noise_on_sphere(imgs)
    lo, hi, valid = pf.noise_bracket(imgs[0], on_sphere)
    assert valid.mean() >= 0.2, float(valid.mean())
    for im in imgs[1:]:
        out = ((im < lo) | (im > hi)).any(axis=-1) & valid
        assert not out.any(), int(out.sum())
