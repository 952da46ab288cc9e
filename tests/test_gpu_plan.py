"""The launch plan as the GPU runs it: every case of tests/golden/launch_plan.json (see
tests/test_launch_plan.py for where its values come from) rendered once at max_depth 8, and
rt_last_stats compared with the recorded values. The file is for the MI355X: the ring's size and
the LDS budget follow the device's CU count and LDS sizes."""
import json
import os

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE, *CASES = [json.loads(line) for line in open(os.path.join(REPO, "tests", "golden", "launch_plan.json"))]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds(rt):
    built = {}

    def get(scene_id):
        if scene_id not in built:
            built[scene_id] = rt.World(1).build_scene(scene_id)
        return built[scene_id]
    return get


def configure(rt, r, c):
    r.set_schedule(c["sched"])
    r.set_precision(c["prec"])
    r.set_variant(c["opt_slab32"], c["opt_lds_stack"], c["opt_lds_nodes"])
    r.set_option(rt.RT_OPT_TRACE_BUF_BYTES, c["buf_bytes"])
    r.set_option(rt.RT_OPT_BATCH_OVERLAP, c["overlap"])
    r.set_option(rt.RT_OPT_BLOCK_SAMPLES, c["block_samples"])
    r.set_option(rt.RT_OPT_BLOCK_CHUNKS, c["block_chunks"])
    r.set_option(rt.RT_OPT_EXTRA_FEATURES, c["extra_features"])
    r.set_option(rt.RT_OPT_POOL_RING, c["ring"])


DEFAULTS = dict(sched=3, prec=0, opt_slab32=1, opt_lds_stack=1, opt_lds_nodes=1, buf_bytes=0, overlap=1, block_samples=0,
                block_chunks=0, extra_features=0, ring=1)   # (a bound of 0: the context's default)


def test_the_golden_file_is_this_devices():
    import torch
    assert torch.cuda.get_device_properties(0).multi_processor_count == DEVICE["n_cus"]


@pytest.mark.parametrize("c", CASES, ids=[c["case"] for c in CASES])
def test_last_stats_match_the_recorded_plan(rt, renderer, worlds, c):
    cam, bg = rt.scene_camera(c["scene"], c["width"], c["height"])
    if c["cam_far"]:   # beyond 2 x the scene's padded extent: no f32 slab tests
        cam.origin[0], cam.origin[1], cam.origin[2] = 1e9, 0.0, 0.0
    p = rt.Renderer.params(c["width"], c["height"], c["spp"], DEVICE["max_depth"], bg, 1, row_begin=c["row_begin"],
                           row_stride=c["row_stride"], spp_chunk=c["spp_chunk"], out_format=rt.RT_OUT_F64,
                           tile_shard=c["tile_shard"])
    try:
        configure(rt, renderer, c)
        renderer.upload(worlds(c["scene"]))
        if c["accum"]:   # one rt_accum_add of all the samples
            acc = renderer.accumulator(p)
            acc.add(cam, p, c["spp"])
            st = renderer.stats().as_dict()
            img = acc.resolve(out_format=rt.RT_OUT_F64)
            acc.close()
        else:
            img = renderer.render(cam, p)
            st = renderer.stats().as_dict()
    finally:
        configure(rt, renderer, DEFAULTS)
    assert np.all(np.isfinite(img))
    diff = {k: (st[k], v) for k, v in c["expect"].items() if st[k] != v}
    assert not diff, "(rt_last_stats, recorded) %s" % diff
