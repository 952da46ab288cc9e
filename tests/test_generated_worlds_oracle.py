"""The generated worlds (tests/generated_worlds.py) on the oracle alone, no GPU: a parity test on
them (tests/test_gpu_generated_worlds.py) is only worth something if the oracle's images are
sound and the views look at what the worlds are about."""
from functools import lru_cache

import numpy as np
import pytest

from tests import generated_worlds as gw

ALL = gw.SUPPORTED + gw.BVH_CASES
_BY_NAME = {c.name: c for c in ALL}


@lru_cache(maxsize=None)
def oracle_image(rt, name, skip=(), threads=1):
    """Rendered once per (world, left-out tags, threads), shared by the tests, read-only."""
    img = gw.oracle_render(rt, _BY_NAME[name], skip=skip, threads=threads)
    img.setflags(write=False)
    return img


@pytest.mark.parametrize("case", ALL, ids=[c.name for c in ALL])
def test_oracle_renders_are_finite_lit_and_thread_independent(rt, case):
    one = oracle_image(rt, case.name)
    assert one.shape == (gw.H, gw.W, 3)
    assert np.all(np.isfinite(one))
    assert float(one.max()) > 0.0 and int(np.count_nonzero(one.sum(axis=2) > 0.0)) >= gw.W * gw.H // 4
    assert np.array_equal(oracle_image(rt, case.name, threads=5), one)


@pytest.mark.parametrize("case", gw.FINDINGS, ids=[c.name for c in gw.FINDINGS])
def test_each_findings_primitives_change_the_oracles_image(rt, case):
    """The oracle with and without the primitives a finding is about, at the size and seed the GPU
    test renders: at least 20 of the 768 pixels differ, so a kernel that missed them would fail
    parity. A condition on the choice of world and view, not a measurement."""
    with_p, without = oracle_image(rt, case.name), oracle_image(rt, case.name, skip=("finding",))
    differ = int(np.count_nonzero(np.any(with_p != without, axis=2)))
    print(f"{case.name}: {differ} of {gw.W * gw.H} pixels differ")
    assert differ >= 20, differ


def test_the_generator_visits_what_it_promises(rt):
    """Counts over the product's tables of the supported family: negative radii, refraction
    indices, fuzz, noise scales, image textures on every material that takes one, every op-chain
    length, shutters on both sides of the camera's, and a camera time range outside [0, 1]."""
    import ctypes
    from tests.test_box_containment import INSTANCE, PRIM, MOVING
    neg, irs, fuzz, scales, chains, shutters, img_mats = 0, set(), set(), set(), set(), set(), set()
    for case in gw.SUPPORTED:
        w = gw.build(rt, case).tw.product
        soa = w.flatten()
        prims = np.frombuffer(ctypes.string_at(soa.prims, soa.n_prims * PRIM.itemsize), dtype=PRIM)
        inst = np.frombuffer(ctypes.string_at(soa.instances, soa.n_instances * INSTANCE.itemsize), dtype=INSTANCE)
        neg += int(np.count_nonzero((prims["kind"] <= MOVING) & (prims["p"][:, 3] < 0)))
        chains |= set(inst["n_ops"].tolist())
        shutters |= {(p["p"][8], p["p"][9]) for p in prims[prims["kind"] == MOVING]}
        mats = np.frombuffer(ctypes.string_at(soa.materials, soa.n_materials * 64), dtype=np.dtype(
            [("kind", "<i4"), ("tex", "<i4"), ("pad", "<i4", (2,)), ("albedo", "<f8", (3,)), ("fuzz", "<f8"), ("ir", "<f8"),
             ("pad2", "<f8")]))
        texs = np.frombuffer(ctypes.string_at(soa.textures, soa.n_textures * 96), dtype=np.dtype(
            [("kind", "<i4"), ("perlin", "<i4"), ("img_w", "<i4"), ("img_h", "<i4"), ("img_offset", "<i8"), ("img_bps", "<i8"),
             ("c0", "<f8", (3,)), ("c1", "<f8", (3,)), ("scale", "<f8"), ("pad", "<f8")]))
        irs |= set(mats["ir"][mats["kind"] == 2].tolist())
        fuzz |= set(mats["fuzz"][mats["kind"] == 1].tolist())
        scales |= set(texs["scale"][texs["kind"] == 2].tolist())
        img_mats |= {int(m["kind"]) for m in mats if m["kind"] in (0, 3, 4) and texs[m["tex"]]["kind"] == 3}
        if case.name.startswith("camera_") and "slab32" in case.name:
            # the f32-slab limit (csrc/launch_plan.cpp): |camera| + its lens against 2 * pad_extent
            assert soa.pad_extent == gw.PAD_EXTENT_EIGHT
            reach = float(np.linalg.norm(case.look_from)) + 0.5 * case.aperture * 3.0
            assert (reach > 2.0 * soa.pad_extent) == (case.name == "camera_beyond_slab32")
            assert abs(reach - 2.0 * soa.pad_extent) < 1.0      # one just outside, one just inside
    assert neg >= 8
    assert {0.5, 1.0, 1.3, 1.5, 2.4} <= irs
    assert {0.0, 0.5, 1.0} <= fuzz and max(fuzz) > 1.0
    assert min(scales) < 1.0 and len(scales - {4.0}) >= 3
    assert img_mats == {0, 3, 4}            # lambertian, light, isotropic
    assert {1, 2, 3, 4} <= chains
    assert {(0.25, 0.75), (0.0, 1.0), (-1.0, 2.0), (2.0, 3.0)} <= shutters
    assert any(min(c.time) < 0.0 or max(c.time) > 1.0 for c in gw.SUPPORTED)
    assert any(c.time != (0.0, 1.0) and 0.0 <= min(c.time) and max(c.time) <= 1.0 for c in gw.SUPPORTED)
