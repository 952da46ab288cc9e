"""The oracle against closed-form transport, per pixel (CPU).

tests/test_oracle.py pins the oracle to the reference by a correlation with two of the reference's
images; nothing there says its transport is right. Here the oracle renders the two-valued worlds of
tests/transport_worlds.py and its per-pixel counts are held to Beer-Lambert, Schlick, the cosine
lobe's view factor and the shutter's coverage, formulas evaluated in numpy that share no code with
oracle.c. This pins the oracle to physics independently of its own code, and proves on the oracle
alone every condition tests/test_gpu_f32_transport.py relies on: the lattice holds exactly, the
closed forms are converged in the sub-pixel grid, the oracle-referenced worlds have the samples
their variance rule needs, and the texel world has the interior pixels the GPU test compares.

Render seed 1 at SPP is the asserted run; seeds 2-4 are printed as evidence at EVIDENCE_SPP (the
time budget). A failure is explained, not re-seeded.
"""
import concurrent.futures as cf
from functools import lru_cache

import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import path_free_worlds as pf
from tests import transport_worlds as tw

CLOSED = tw.closed_form_worlds()
REF = tw.oracle_ref_worlds()
THREADS = 16
EVIDENCE_SPP = 4096


def _renders(spec, spp, seeds):
    w = ob.OracleWorld(1)
    try:
        spec.build(w)
        return [w.render(spec.cam24(), pf.BG, spec.W, spec.H, spp, render_seed=s, threads=THREADS) for s in seeds]
    finally:
        w.close()


@lru_cache(maxsize=None)
def _closed_forms(k):
    """name -> p at a k x k grid for every closed-form world (numpy releases the GIL: one thread per world)."""
    with cf.ThreadPoolExecutor(max_workers=THREADS) as ex:
        return dict(zip([s.name for s in CLOSED], ex.map(lambda s: tw.pixel_p(s, k), CLOSED)))


def test_closed_forms_are_converged_in_the_subpixel_grid():
    for spec in CLOSED:
        p, p2 = _closed_forms(tw.K)[spec.name], _closed_forms(2 * tw.K)[spec.name]
        assert p.shape == (spec.H, spec.W) and np.all((p >= 0.0) & (p <= 1.0)), spec.name
        moved = float(np.abs(p2 - p).max())
        print(f"{spec.name}: K = {2 * tw.K} moves p by at most {moved:.2e}; p in [{p.min():.4f}, {p.max():.4f}]")
        assert moved <= 1e-4, (spec.name, moved)
        assert tw.variance(p, tw.SPP).sum() >= 1e5, spec.name      # a world that is all 0 or 1 tests nothing


@pytest.mark.parametrize("name", ["lobe", "absorb-0.7", "schlick-1.5"])
def test_statistics_pass_binomial_counts_and_see_a_one_percent_bias(name):
    """numpy's own binomial draws from the closed form stay inside the bars; the dark chance
    scaled by 1.01 leaves them by a factor of three."""
    p = _closed_forms(tw.K)[name]
    rng = np.random.default_rng(7)
    st = tw.statistics(rng.binomial(tw.SPP, p), p, tw.SPP)
    assert tw.failures(st) == [], tw.describe(name, st)
    st = tw.statistics(rng.binomial(tw.SPP, 1.0 - 1.01 * (1.0 - p)), p, tw.SPP)
    assert abs(st["z_total"]) >= 15.0, tw.describe(name, st)


def test_bins_merge_up_to_the_variance_floor():
    p = np.concatenate([np.full(700, 1.0), np.full(68, 0.5)]).reshape(24, 32)
    j = np.round(tw.SPP * p).astype(np.int64)
    z = tw.z_bins(j, p, tw.SPP)
    assert len(z) == 1 and z[0] == 0.0       # nine bins without variance merge into the one that has it
    assert tw.chi2(j, p, tw.SPP)[2] == 68


@pytest.mark.parametrize("spec", CLOSED, ids=[s.name for s in CLOSED])
def test_oracle_meets_the_closed_form(spec):
    p = _closed_forms(tw.K)[spec.name]
    img = _renders(spec, tw.SPP, [1])[0]
    ok, j = tw.bright_count(img, spec, tw.SPP, 1e-9)
    st = tw.statistics(j, p, tw.SPP)
    print(tw.describe(f"{spec.name} seed 1, {tw.SPP} spp", st) + f", lattice deviation {tw.lattice_dev(img, spec, tw.SPP):.1e}")
    for seed, im in zip((2, 3, 4), _renders(spec, EVIDENCE_SPP, (2, 3, 4))):
        print(tw.describe(f"{spec.name} seed {seed}, {EVIDENCE_SPP} spp",
                          tw.statistics(tw.bright_count(im, spec, EVIDENCE_SPP, 1e-9)[1], p, EVIDENCE_SPP)))
    assert ok.all(), f"{spec.name}: {int((~ok).sum())} pixels off the lattice"
    assert tw.failures(st) == [], tw.describe(spec.name, st)


@pytest.mark.parametrize("spec", REF, ids=[s.name for s in REF])
def test_oracle_referenced_worlds_have_the_samples_the_variance_rule_needs(spec):
    """The pool is two-valued at every seed and 8 x SPP samples per pixel, so its variance is 1/8
    of one run's; a further seed of the oracle meets the bars against it."""
    p, n, ok = tw.pooled_p(_renders(spec, tw.SPP, tw.REF_SEEDS), spec, tw.SPP, 1e-9)
    assert ok.all(), f"{spec.name}: {int((~ok).sum())} pixels off the lattice"
    assert n >= 8 * tw.SPP
    assert tw.variance(p, tw.SPP).sum() >= 1e5, spec.name
    img = _renders(spec, tw.SPP, [1])[0]
    ok, j = tw.bright_count(img, spec, tw.SPP, 1e-9)
    st = tw.statistics(j, p, tw.SPP, n)
    print(tw.describe(f"{spec.name} seed 1 against the pool", st))
    assert ok.all() and tw.failures(st) == [], tw.describe(spec.name, st)


def test_texel_world_has_interior_pixels_of_most_texels():
    spec = tw.texel_world()
    imgs = _renders(spec, spec.spp, pf.SEEDS)
    inner = pf.interior(imgs)
    assert float(inner.mean()) >= spec.min_share, float(inner.mean())
    known = np.all(np.abs(imgs[0] - np.asarray(pf.BG)) <= 1e-12, axis=-1)
    for c, _ in spec.owners:
        known |= np.all(np.abs(imgs[0] - np.asarray(c)) <= 1e-12, axis=-1)
    assert known[inner].all()
    owning = pf.colours_owning(imgs[0], inner, spec.owners)
    print(f"{spec.name}: interior share {float(inner.mean()):.3f}, {owning} of {len(spec.owners)} texels own an interior pixel")
    assert owning >= len(spec.owners) // 2      # the sphere shows half of its texels, the rect all of its
