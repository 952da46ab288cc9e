"""The f32 fast mode (RT_PREC_F32) held to the oracle per pixel.

The f32 kernels draw and round differently, so their paths are not the oracle's; on the
path-independent worlds of tests/path_free_worlds.py the pixel does not depend on the path,
and every f32 instantiation (csrc/trace_f32_*.hip, under each schedule's kernel) must give
the oracle's pixel to rounding. tests/test_path_free_worlds.py shows on the CPU that the
oracle itself meets every condition used here. The f64 path renders the same worlds to the
parity bar of tests/test_gpu_parity.py (path identity at grazing incidence, |p| ~ 1000 and
r around the f32 small-sphere threshold).

Tolerances (none measured on the kernels): an f32 sample a*bg carries a relative error of at
most 3 * 2^-24 = 2e-7, so |dj| <= 2e-7 * spp / (1 - 0.5) = 3.2e-6 at 8 spp against the 1e-4
used, while one re-hit moves j by >= 0.3; an emitter colour <= 1 rounds to f32 within 6e-8
against the 1e-6 used. Caps: off-lattice pixels <= max(1, 1e-3 W H spp) (the oracle: 0),
black furnace samples <= 1e-3 of the samples (the oracle: <= 1e-4), ID exceptions: none.
"""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import path_free_worlds as pf
from tests.test_gpu_nesting import _cam24
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

ONE_BOUNCE = pf.one_bounce_worlds()
ID_WORLDS = pf.id_worlds()
J_TOL = 1e-4

_twins = {}


def _twin(rt, spec):
    """The world in the product and the oracle, its camera, and the oracle's renders at the
    four seeds: built once per world and shared by the tests that use it."""
    if spec.name not in _twins:
        tw = ob.TwinWorld(rt, 1)
        spec.build(tw)
        cam = rt.camera_new(spec.look_from, spec.look_at, spec.vup, spec.vfov, spec.W / spec.H, 0.0, 10.0, 0.0, 1.0)
        assert np.allclose(_cam24(cam), spec.cam24(), rtol=0, atol=1e-9)     # the CPU file's camera
        refs = [tw.oracle.render(_cam24(cam), pf.BG, spec.W, spec.H, spec.spp, render_seed=s) for s in pf.SEEDS]
        _twins[spec.name] = (tw, cam, refs)
    return _twins[spec.name]


SCHEDULES = {"auto": ("RT_SCHED_AUTO", None), "chunks": ("RT_SCHED_CHUNKS", None), "pool-ring0": ("RT_SCHED_POOL", 0),
             "pool-ring2": ("RT_SCHED_POOL", 2), "items": ("RT_SCHED_ITEMS", None), "count": ("RT_SCHED_AUTO", None)}


def _render(rt, renderer, spec, precision, sched="auto"):
    """One render of the world through the session's renderer under a precision and a
    schedule ('count': the count_work kernel); options, schedule and precision restored."""
    tw, cam, _ = _twin(rt, spec)
    sched_name, ring = SCHEDULES[sched]
    ring0 = renderer.get_option(rt.RT_OPT_POOL_RING)
    extra0 = renderer.get_option(rt.RT_OPT_EXTRA_FEATURES)
    try:
        renderer.set_option(rt.RT_OPT_EXTRA_FEATURES, spec.extra)
        renderer.set_precision(precision)
        renderer.set_schedule(getattr(rt, sched_name))
        if ring is not None:
            renderer.set_option(rt.RT_OPT_POOL_RING, ring)
        renderer.upload(tw.product)
        img = renderer.render(cam, rt.Renderer.params(spec.W, spec.H, spec.spp, 50, pf.BG, 1, out_format=rt.RT_OUT_F64,
                                                      count_work=int(sched == "count")))
        st = renderer.stats()
    finally:
        renderer.set_schedule(rt.RT_SCHED_AUTO)
        renderer.set_option(rt.RT_OPT_POOL_RING, ring0)
        renderer.set_precision(rt.RT_PREC_F64)
        renderer.set_option(rt.RT_OPT_EXTRA_FEATURES, extra0)
    assert st.precision == precision and st.variant_features == spec.features, (spec.name, st.precision, st.variant_features)
    if sched not in ("auto", "count"):
        assert st.schedule == getattr(rt, sched_name), (spec.name, sched, st.schedule)
    if ring is not None:
        assert (st.ring_bytes > 0) == (ring == 2), (spec.name, sched, st.ring_bytes)
    assert np.all(np.isfinite(img)), f"{spec.name} [{sched}]: non-finite pixels"
    _render.stats = st
    return img


def _f64_matches_oracle(rt, renderer, spec, sched="auto"):
    img = _render(rt, renderer, spec, rt.RT_PREC_F64, sched)
    assert_parity(img, _twin(rt, spec)[2][0], f"{spec.name} [{sched}] f64")


def _worst(err):
    y, x = np.unravel_index(int(np.argmax(err)), err.shape)
    return int(y), int(x)


def _check_one_bounce(rt, renderer, spec, sched="auto"):
    _f64_matches_oracle(rt, renderer, spec, sched)
    img = _render(rt, renderer, spec, rt.RT_PREC_F32, sched)
    refs = _twin(rt, spec)[2]
    W, H, spp, a = spec.W, spec.H, spec.spp, spec.albedo
    tag = f"{spec.name} [{sched}] f32"
    ok, j = pf.lattice_j(img, pf.BG, a, spp, J_TOL)

    def at(y, x):
        return f"pixel (row {y}, col {x}) j per channel {pf.channel_j(img[y, x], pf.BG, a, spp)}"

    jc = pf.channel_j(img, pf.BG, a, spp)
    dev = np.abs(jc - np.rint(jc[..., :1])).max(axis=-1)
    n_off = int((~ok).sum())
    print(f"{tag}: {n_off} off-lattice pixels of {W * H}, worst |dj| {float(dev.max()):.3e}")
    assert n_off <= max(1, int(1e-3 * W * H * spp)), f"{tag}: {n_off} off-lattice pixels, worst {at(*_worst(dev))}"
    js = [pf.lattice_j(r, pf.BG, a, spp, 1e-9)[1] for r in refs]
    full, none = pf.settled(js, spp), pf.settled(js, 0)
    if a is None:
        none, full = np.ones((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    for mask, want in ((full, spp), (none, 0)):
        bad = mask & ((j != want) | ~ok)
        assert not bad.any(), (f"{tag}: {int(bad.sum())} pixels where every oracle seed has j = {want} on the 3x3 "
                               f"neighbourhood, worst {at(*_worst(np.where(bad, np.abs(jc - want).max(axis=-1), -1.0)))}")
    edge = int((~(full | none)).sum())
    diff = abs(int(np.clip(j, 0, spp).sum()) - int(js[0].sum()))
    assert diff <= edge * spp, f"{tag}: coverage differs by {diff} samples with {edge} non-interior pixels"


def _check_id(rt, renderer, spec, sched="auto"):
    _f64_matches_oracle(rt, renderer, spec, sched)
    img = _render(rt, renderer, spec, rt.RT_PREC_F32, sched)
    tw, _, refs = _twin(rt, spec)
    if spec.n_spheres:      # the partial-TLAS instantiation: more TLAS nodes than the block keeps in LDS
        assert 0 < _render.stats.lds_nodes < tw.product.flatten().n_tlas_nodes
    inner = pf.interior(refs)
    assert inner.mean() >= spec.min_share, (spec.name, float(inner.mean()))
    err = np.where(inner, np.abs(img - refs[0]).max(axis=-1), 0.0)
    y, x = _worst(err)
    print(f"{spec.name} [{sched}] f32: {int(inner.sum())} interior pixels, worst |f32 - oracle| {float(err.max()):.3e}")
    assert float(err.max()) <= 1e-6, (f"{spec.name} [{sched}] f32: {int((err > 1e-6).sum())} interior pixels differ, worst "
                                      f"pixel (row {y}, col {x}) {img[y, x]} against the oracle's {refs[0][y, x]}")


def _check_furnace(rt, renderer, spec, sched="auto"):
    _f64_matches_oracle(rt, renderer, spec, sched)
    img = _render(rt, renderer, spec, rt.RT_PREC_F32, sched)
    tag = f"{spec.name} [{sched}] f32"
    jc = (1.0 - img / np.asarray(pf.BG)) * spec.spp
    dev = np.abs(jc - np.rint(jc[..., :1])).max(axis=-1)
    ok, n_black = pf.furnace_black(img, pf.BG, spec.spp, J_TOL)
    y, x = _worst(dev)
    share = n_black / (spec.W * spec.H * spec.spp)
    print(f"{tag}: {int((~ok).sum())} pixels off the lattice, worst |dj| {float(dev.max()):.3e}, black share {share:.3e}")
    assert ok.all(), f"{tag}: {int((~ok).sum())} pixels off the black-sample lattice, worst pixel (row {y}, col {x}) j per channel {jc[y, x]}"
    over = img > np.asarray(pf.BG) * (1.0 + 1e-6)
    assert not over.any(), f"{tag}: {int(over.any(axis=-1).sum())} pixels brighter than the background"
    assert share <= 1e-3, f"{tag}: black samples {n_black} ({share} of the samples)"


@pytest.mark.parametrize("spec", ONE_BOUNCE, ids=[s.name for s in ONE_BOUNCE])
def test_one_bounce_worlds_sit_on_the_oracles_lattice(rt, renderer, spec):
    """Every sample is bg or a*bg: the f32 pixel is on the lattice, full where the oracle is
    full, empty where it is empty, and covers what the oracle covers. A ray that re-hits the
    surface it leaves (the surface offset), a far root taken for the near one or a c = |oc|^2 -
    r^2 lost to cancellation all leave the lattice."""
    _check_one_bounce(rt, renderer, spec)


@pytest.mark.parametrize("full", [True, False], ids=["all", "media"])
def test_furnace_returns_the_background(rt, renderer, full):
    """Albedo 1 everywhere: a sample is bg, or black when its path never escapes. A skipped
    medium boundary, a NaN from the dielectric branch or an energy gain shows as a pixel off
    the lattice or above bg; paths trapped by re-hits as black samples."""
    _check_furnace(rt, renderer, pf.furnace_world(full))


@pytest.mark.parametrize("spec", ID_WORLDS, ids=[s.name for s in ID_WORLDS])
def test_id_worlds_show_the_oracles_first_hit(rt, renderer, spec):
    """Every primitive emits its own colour: an interior pixel (3x3 pure over four oracle
    seeds) is the first hit's colour in any renderer. A missed node of the f32 walk, a wrong
    root, a wrong checker parity or a wrong instance transform changes a colour. The big field
    takes the spheres variant's partial-TLAS instantiation (32-bit stack)."""
    _check_id(rt, renderer, spec)


def _by_name(specs, name):
    return next(s for s in specs if s.name == name)


@pytest.mark.parametrize("sched", ["chunks", "pool-ring0", "pool-ring2", "items", "count"])
@pytest.mark.parametrize("variant", ["spheres", "final"])
def test_every_schedules_kernel_on_the_spheres_and_final_sets(rt, renderer, variant, sched):
    """Each schedule compiles the contracted f32 path code on its own (and count_work its own
    translation unit): one ID world and one one-bounce world per kernel."""
    id_name, ob_name = {"spheres": ("id-spheres", "grazing-far-lambertian"), "final": ("id-final", "box1000-lambertian")}[variant]
    _check_id(rt, renderer, _by_name(ID_WORLDS, id_name), sched)
    _check_one_bounce(rt, renderer, _by_name(ONE_BOUNCE, ob_name), sched)


def test_noise_emitter_lies_in_the_oracles_bracket(rt, renderer):
    """The f32 Perlin marble at the first hit: each channel within [min, max] of the oracle's
    5x5 neighbourhood, widened by 1e-3, no exceptions (the oracle's other seeds have none)."""
    spec = pf.noise_world()
    _f64_matches_oracle(rt, renderer, spec)
    img = _render(rt, renderer, spec, rt.RT_PREC_F32)
    refs = _twin(rt, spec)[2]
    lo, hi, valid = pf.noise_bracket(refs[0], pf.noise_on_sphere(refs))
    assert valid.mean() >= 0.2
    out = ((img < lo) | (img > hi)).any(axis=-1) & valid
    y, x = _worst(np.where(valid, np.maximum(lo - img, img - hi).max(axis=-1), -1.0))
    assert not out.any(), (f"{int(out.sum())} pixels outside the bracket, worst (row {y}, col {x}) {img[y, x]} "
                           f"against [{lo[y, x]}, {hi[y, x]}]")


@pytest.mark.parametrize("scene_id,W,H,spp,mean_tol", [
    (0, 64, 48, 64, 0.01),     # random spheres (C1/C2/C5)
    (5, 48, 48, 128, 0.02),    # Cornell box (C3)
    (7, 64, 32, 96, 0.03),     # final scene (C4)
])
def test_f32_mode_agrees_with_the_oracle_statistically(rt, renderer, scene_id, W, H, spp, mean_tol):
    """tests/test_gpu_f32.py::test_f32_mode_agrees_statistically with the reference
    distribution from the oracle (render seeds 1..8) instead of f64 GPU renders: the same
    scenes, sizes, spp, t-statistic bounds and mean tolerances."""
    ref = [ob.render(scene_id, W, H, spp, 50, render_seed=s) for s in range(1, 9)]
    renderer.set_precision(rt.RT_PREC_F32)
    try:
        f32, st = rt.render_scene(scene_id, W, H, spp, 50, render_seed=1, out_format=rt.RT_OUT_F64, renderer=renderer)
    finally:
        renderer.set_precision(rt.RT_PREC_F64)
    assert st.precision == rt.RT_PREC_F32
    assert np.all(np.isfinite(f32)) and f32.min() >= 0.0

    def blocks(x):
        return x.reshape(H // 8, 8, W // 8, 8, 3).mean(axis=(1, 3))

    bm = np.stack([blocks(x) for x in ref])
    sd = bm[1:].std(axis=0, ddof=1)
    se = np.sqrt(2.0) * np.maximum(sd, 1e-6)
    t = np.abs(blocks(f32) - bm[0]) / se
    print(f"scene {scene_id}: mean |t| {float(np.mean(t)):.3f}, blocks with |t| > 6: {int(np.sum(t > 6.0))}, "
          f"mean ratio {float(f32.mean()) / float(np.mean(ref)):.5f}")
    assert float(np.mean(t)) < 1.5, float(np.mean(t))
    assert int(np.sum(t > 6.0)) <= 2, int(np.sum(t > 6.0))
    mean = float(np.mean(ref))
    assert abs(float(f32.mean()) / mean - 1.0) < mean_tol, (float(f32.mean()), mean)
