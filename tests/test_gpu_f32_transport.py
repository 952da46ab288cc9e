"""The f32 fast mode's sampling (RT_PREC_F32) held to closed-form transport per pixel.

The path-independent worlds of tests/test_gpu_f32_exact.py cannot see how the f32 kernels sample:
their pixels do not depend on the direction, distance or time drawn. On the two-valued worlds of
tests/transport_worlds.py the pixel is an integer count j ~ Binomial(spp, p), with p from
Beer-Lambert, Schlick, the cosine lobe's view factor or the shutter's coverage in f64 numpy, so the
Lambertian lobe, the dielectric's reflect / refract choice, the medium's -1/rho logf(u) free path
with its re-entry step, and the shutter draw with the moving centre are each held per pixel, on top
of the fast division, v_rsq_f32, contracted FMAs, 24-bit uniforms and Philox-7 that only the f32
units have. tests/test_transport_worlds.py shows on the CPU that the oracle meets the same bars.

Per world: the f64 kernel to the parity bar against the oracle at 8 spp (the world runs on the
intended variant and path for path), then the f32 kernel at SPP = 16384 spp, render seed 1: no
pixel off the lattice (tolerance: TSpec.j_tol, 32 x the f32 rounding bound) and |z| <= 5 on the
total count, on the bins of pixels ordered by p and on chi^2. The oracle-referenced worlds
(oracle-ref/...) are barred against the oracle's pooled counts with the pool's variance added.
None of the bars is measured on the kernels.
"""
import dataclasses

import numpy as np
import pytest

from tests import path_free_worlds as pf
from tests import oracle_binding as ob
from tests import test_gpu_f32_exact as ex
from tests import transport_worlds as tw
from tests.test_gpu_f32_exact import SCHEDULES, _render, _twin
from tests.test_gpu_nesting import _cam24
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

CLOSED = tw.closed_form_worlds()
REF = tw.oracle_ref_worlds()
WORLDS = CLOSED + REF
THREADS = 16

_p = {}


def _world(rt, spec):
    """tests/test_gpu_f32_exact._twin; a world whose camera has an aperture or its own shutter is
    entered into the same table with that camera."""
    if spec.name not in ex._twins and (spec.aperture, spec.time0, spec.time1) != (0.0, 0.0, 1.0):
        t = ob.TwinWorld(rt, 1)
        spec.build(t)
        cam = rt.camera_new(spec.look_from, spec.look_at, spec.vup, spec.vfov, spec.W / spec.H, spec.aperture, 10.0,
                            spec.time0, spec.time1)
        assert np.allclose(_cam24(cam), spec.cam24(), rtol=0, atol=1e-9)
        refs = [t.oracle.render(_cam24(cam), pf.BG, spec.W, spec.H, spec.spp, render_seed=s) for s in pf.SEEDS]
        ex._twins[spec.name] = (t, cam, refs)
    return _twin(rt, spec)


def _expectation(rt, spec):
    """(p, ref_samples): the closed form, or the oracle's pooled share and its sample count."""
    if spec.name not in _p:
        if spec.prob is not None:
            _p[spec.name] = (tw.pixel_p(spec), None)
        else:
            t, cam, _ = _world(rt, spec)
            imgs = [t.oracle.render(_cam24(cam), pf.BG, spec.W, spec.H, tw.SPP, render_seed=s, threads=THREADS)
                    for s in tw.REF_SEEDS]
            p, n, ok = tw.pooled_p(imgs, spec, tw.SPP, 1e-9)
            assert ok.all() and n >= 8 * tw.SPP, spec.name
            _p[spec.name] = (p, n)
    return _p[spec.name]


def _render_f32(rt, renderer, spec, sched):
    """The ring runs only when a pool block is one chunk; a frame this small has its blocks cut to
    4 samples otherwise, so the ring case passes the chunk (16 at SPP) as the block."""
    block0 = renderer.get_option(rt.RT_OPT_BLOCK_SAMPLES)
    try:
        if sched == "pool-ring2":
            renderer.set_option(rt.RT_OPT_BLOCK_SAMPLES, 16)
        return _render(rt, renderer, spec, rt.RT_PREC_F32, sched)
    finally:
        renderer.set_option(rt.RT_OPT_BLOCK_SAMPLES, block0)


def _check(rt, renderer, spec, sched="auto"):
    _world(rt, spec)
    f64 = _render(rt, renderer, spec, rt.RT_PREC_F64, sched)
    assert_parity(f64, _twin(rt, spec)[2][0], f"{spec.name} [{sched}] f64")
    p, n = _expectation(rt, spec)
    img = _render_f32(rt, renderer, dataclasses.replace(spec, spp=tw.SPP), sched)
    tag = f"{spec.name} [{sched}{', all features' if spec.extra == tw.ALL else ''}] f32"
    ok, j = tw.bright_count(img, spec, tw.SPP, spec.j_tol)
    st = tw.statistics(j, p, tw.SPP, n)
    print(tw.describe(tag, st) + f"; {int((~ok).sum())} pixels off the lattice, worst |dj| {tw.lattice_dev(img, spec, tw.SPP):.2e}")
    if not ok.all():
        y, x = np.argwhere(~ok)[0]
        ratio = np.asarray(spec.dark) / np.asarray(spec.bright)
        raise AssertionError(f"{tag}: {int((~ok).sum())} pixels off the lattice, first (row {y}, col {x}) dark count per "
                             f"channel {pf.channel_j(img[y, x], spec.bright, ratio, tw.SPP)}")
    assert tw.failures(st) == [], tw.describe(tag, st)


@pytest.mark.parametrize("spec", WORLDS, ids=[s.name for s in WORLDS])
def test_f32_counts_follow_the_closed_form(rt, renderer, spec):
    """Under AUTO, on the variant the world selects. A biased lobe, free path, Schlick chance or
    shutter time moves the total count; one that depends on the angle or the chord moves a bin; a
    draw that is correlated between samples, or a pixel mapped to the wrong ray, moves chi^2."""
    _check(rt, renderer, spec)


@pytest.mark.parametrize("spec", WORLDS, ids=[s.name for s in WORLDS])
def test_f32_counts_on_the_all_features_variant(rt, renderer, spec):
    """The same worlds through trace_f32_all (RT_OPT_EXTRA_FEATURES = 4095)."""
    _check(rt, renderer, dataclasses.replace(spec, extra=tw.ALL, features=tw.ALL))


def _by_name(name):
    return next(s for s in CLOSED if s.name == name)


@pytest.mark.parametrize("sched", ["chunks", "pool-ring0", "pool-ring2", "items"])
@pytest.mark.parametrize("name", ["absorb-0.7", "absorb-0.7-rotbox", "lobe", "schlick-1.5"])
def test_every_schedules_kernel_samples_alike(rt, renderer, name, sched):
    """Each schedule compiles the f32 path code on its own: the medium (sphere-bounded and
    instanced-box-bounded), the lobe and the dielectric under each trace kernel."""
    assert sched in SCHEDULES
    _check(rt, renderer, _by_name(name), sched)


def test_texel_world_shows_the_oracles_texels(rt, renderer):
    """The f32 u, v -> texel mapping on a sphere (uv from the normal) and a rect (uv stored at the
    hit): interior pixels are the oracle's texel, no exceptions."""
    ex._check_id(rt, renderer, tw.texel_world())
