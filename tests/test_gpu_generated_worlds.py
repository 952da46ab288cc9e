"""The generated twin worlds (tests/generated_worlds.py) on the GPU against the oracle, at 32x24
and 4 spp. The bar is tests/test_gpu_parity.py's assert_parity: L_inf <= 1e-3 and path identity
(relative 1e-9). That the oracle's images are sound and that the views look at the findings'
primitives is checked without a GPU in tests/test_generated_worlds_oracle.py.

For every input the constructors accept the product renders what the oracle renders, or refuses
with a message before any launch and leaves the context usable; it never renders another image.
"""
import numpy as np
import pytest

from tests import generated_worlds as gw
from tests.test_generated_worlds_oracle import oracle_image
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu


def _params(rt, case):
    return rt.Renderer.params(gw.W, gw.H, gw.SPP, 50, case.bg, 1, out_format=rt.RT_OUT_F64)


def _render(rt, renderer, case, accel=None, world=None):
    world = gw.build(rt, case).tw.product if world is None else world
    renderer.upload(world, rt.RT_ACCEL_SAH if accel is None else accel)
    return renderer.render(gw.camera(rt, case), _params(rt, case))


@pytest.fixture(scope="module")
def all_features(rt):
    big = rt.Renderer(0)
    big.set_option(rt.RT_OPT_EXTRA_FEATURES, 4095)
    yield big
    big.close()


@pytest.mark.parametrize("case", gw.SUPPORTED, ids=[c.name for c in gw.SUPPORTED])
def test_generated_world_matches_oracle(rt, renderer, case):
    got = _render(rt, renderer, case)
    if case.name == "camera_beyond_slab32":      # |camera| > 2 * pad_extent: the f64 slab tests
        assert renderer.stats().slab32 == 0
    if case.name == "camera_within_slab32":
        assert renderer.stats().slab32 == 1
    assert_parity(got, oracle_image(rt, case.name), case.name)


@pytest.mark.parametrize("case", gw.UNBOUNDED_BY_REFERENCE, ids=[c.name for c in gw.UNBOUNDED_BY_REFERENCE])
def test_finding_worlds_render_the_same_bits_in_every_hierarchy_and_variant(rt, renderer, all_features, case):
    """SAH, LINEAR (no box gates anything) and MEDIAN render the same bits, and the all-features
    variant (RT_OPT_EXTRA_FEATURES) the bits of the variant the world selects."""
    world = gw.build(rt, case).tw.product
    sah = _render(rt, renderer, case, rt.RT_ACCEL_SAH, world)
    selected = renderer.stats().variant_features
    for accel in (rt.RT_ACCEL_LINEAR, rt.RT_ACCEL_MEDIAN):
        assert np.array_equal(_render(rt, renderer, case, accel, world), sah), (case.name, accel)
    big = _render(rt, all_features, case, rt.RT_ACCEL_SAH, world)
    assert all_features.stats().variant_features == 4095
    assert np.array_equal(big, sah), (case.name, selected)
    assert_parity(sah, oracle_image(rt, case.name), case.name)


@pytest.mark.parametrize("case", gw.BVH_CASES, ids=[c.name for c in gw.BVH_CASES])
def test_bvh_over_unbounded_children_is_refused_or_equal(rt, renderer, case):
    """rt_world_bvh over children whose reference box does not bound them: exactly two outcomes.
    Refused with RT_ERR_UNSUPPORTED at upload, the context still rendering the next world; or
    rendered as the oracle renders it."""
    try:
        got = _render(rt, renderer, case)
    except rt.RTError as e:
        assert "RT_ERR_UNSUPPORTED" in str(e) and "rt_world_bvh node" in str(e), str(e)
        other = gw.SUPPORTED[0]
        assert_parity(_render(rt, renderer, other), oracle_image(rt, other.name), f"{other.name} after a refusal")
        return
    assert_parity(got, oracle_image(rt, case.name), case.name)


def test_camera_shutter_outside_the_built_time_range_is_refused_and_the_context_lives(rt, renderer):
    """The shutters world is built for ray times [0, 1]. A camera with time1 = 1.5 is refused by
    every pass before any launch (csrc/launch_plan.cpp), and the same context then renders the
    world under its own camera as the oracle does. Built for [0, 1.5] it renders."""
    case = next(c for c in gw.SUPPORTED if c.name == "shutters")
    b = gw.build(rt, case)
    renderer.upload(b.tw.product)
    late = rt.camera_new(case.look_from, case.look_at, (0.0, 1.0, 0.0), case.vfov, gw.W / gw.H, case.aperture, case.focus,
                         0.0, 1.5)
    for call in (renderer.render, renderer.render_features):
        with pytest.raises(rt.RTError, match="RT_ERR_UNSUPPORTED.*time range"):
            call(late, _params(rt, case))
    assert_parity(renderer.render(gw.camera(rt, case), _params(rt, case)), oracle_image(rt, case.name), "after the refusal")
    b.tw.product.set_build_option(rt.RT_BUILD_TIME1, 1.5)
    renderer.upload(b.tw.product)
    got = renderer.render(late, _params(rt, case))
    ref = b.tw.oracle.render(gw.cam24(late), case.bg, gw.W, gw.H, gw.SPP)
    assert_parity(got, ref, "built for [0, 1.5]")
