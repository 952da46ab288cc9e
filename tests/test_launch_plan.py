"""The launch plan (csrc/launch_plan.cpp: kernel configuration, schedule, buffer batches and
their memory) pinned on the CPU.

tests/plan_dump.cpp links the scene builders, the flattener, the lowering and the plan — nothing
from HIP — reads the cases of tests/golden/launch_plan.json and prints what rtp::plan decides
for each. It is built with ASan and UBSan (the program itself is instrumented, so nothing is
preloaded).

The golden file's "expect" values are rt_last_stats of commit 4fc25f7 (source hash
41556f322068adba, the file's "recorded_from"), the last one whose run_range still held this
logic inline, after rendering each case on an MI355X at max_depth 8; its first line holds that
device's CU count and LDS sizes, read in the same run. Every case sets RT_OPT_TRACE_BUF_BYTES, so
free device memory played no part. They were never taken from rtp::plan's own output: do not
regenerate them from plan_dump. tests/test_gpu_plan.py renders the same cases on the GPU.
"""
import json
import os
import subprocess

import pytest

from tests.test_lowering import LOWERING_SOURCES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust-ray-tracing-in-a-weekend_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "launch_plan.json")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-ffp-contract=off"]
SOURCES = [os.path.join(REPO, "tests", "plan_dump.cpp")] + LOWERING_SOURCES + [os.path.join(CSRC, "launch_plan.cpp")]
MIB = 1 << 20
POOL, ITEMS, AUTO = 1, 2, 3
DEFAULTS = dict(spp_chunk=0, row_begin=0, row_stride=1, tile_shard=0, sched=AUTO, prec=0, ring=1, overlap=1,
                block_samples=0, block_chunks=0, extra_features=0, opt_slab32=1, opt_lds_stack=1, opt_lds_nodes=1,
                cam_far=0, accum=0, buf_bytes=1 << 30)


def golden():
    """(device facts, cases) of the golden file."""
    lines = [json.loads(line) for line in open(GOLDEN)]
    return lines[0], lines[1:]


@pytest.fixture(scope="module")
def plan_dump(tmp_path_factory):
    """Builds plan_dump once (no HIP include path, no HIP library); returns run(case file) -> its lines."""
    exe = str(tmp_path_factory.mktemp("plan_dump") / "plan_dump")
    b = subprocess.run([CLANG, *FLAGS, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]

    def run(case_file):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        r = subprocess.run([exe, case_file], capture_output=True, text=True, env=env, timeout=120)
        report = r.stdout + r.stderr
        assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
        assert r.returncode == 0, report[-4000:]
        return [json.loads(line) for line in r.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def attempts(plan_dump):
    """Every attempt plan_dump prints for the golden file's cases, by case name."""
    out = {}
    for a in plan_dump(GOLDEN):
        out.setdefault(a["case"], []).append(a)
    return out


def test_plan_matches_the_parents_stats_under_asan_and_ubsan(attempts):
    _, cases = golden()
    assert list(attempts) == [c["case"] for c in cases]
    for c in cases:
        got = [a for a in attempts[c["case"]] if a["primary"]]
        assert len(got) == 1 and got[0]["bound"] == c["buf_bytes"] and got[0]["err"] == 0, c["case"]
        diff = {k: (got[0][k], v) for k, v in c["expect"].items() if got[0][k] != v}
        assert not diff, "%s: (plan, parent's rt_last_stats) %s" % (c["case"], diff)


def test_golden_covers_what_the_project_states():
    """The figures the documents and the GPU tests quote, read from the golden file itself."""
    c = {w["case"]: w["expect"] for w in golden()[1]}
    # 64x48x40 under a 1 MiB bound (tests/test_gpu_parity.py): the Cornell variants' 256-thread
    # workgroups overlap 5 x 7 + 5 samples, the random and final scenes' run 14 + 14 + 12 in order
    for s in (0, 7):
        assert (c["pool_inorder_s%d" % s]["n_batches"], c["pool_inorder_s%d" % s]["overlapped"]) == (3, 0)
    for s in (5, 6):
        assert (c["pool_overlap_s%d" % s]["n_batches"], c["pool_overlap_s%d" % s]["overlapped"]) == (6, 1)
    for s in (0, 5, 6, 7):
        assert (c["pool_serial_s%d" % s]["n_batches"], c["pool_serial_s%d" % s]["overlapped"]) == (3, 0)
    assert c["items_chunk_batches_s5"]["n_batches"] == 12 and c["accum_items_s5"]["n_batches"] == 12
    # AUTO: the item pool for the Cornell box in f64, the per-sample pool otherwise, the item pool
    # again when the samples are more than 4 bounds and no ring can take them
    assert [c["auto_s%d" % s]["schedule"] for s in (0, 5, 6, 7)] == [POOL, ITEMS, POOL, POOL]
    assert c["auto_s5_f32"]["schedule"] == POOL and c["auto_s0_200spp_items"]["schedule"] == ITEMS
    # RT_OPT_POOL_RING 2 / 1 / 0
    assert c["ring_always_s0"]["ring_bytes"] > 0 and c["ring_never_s0"]["ring_bytes"] == 0
    assert c["ring_when_needed_fits_s0"]["ring_bytes"] == 0 and c["ring_when_needed_nofit_s0"]["ring_bytes"] > 0
    # batches beside the ring: one ring in order (final scene), two when overlapped (Cornell box)
    s7, s5 = c["ring_batches_s7"], c["ring_batches_s5"]
    assert s7["n_batches"] == 3 and s5["n_batches"] == 3 and (s7["overlapped"], s5["overlapped"]) == (0, 1)
    assert s5["ring_bytes"] == 2 * s7["ring_bytes"]
    # LDS staging, slab32, the empty shard, the accumulator
    assert c["lds_default_s0"]["lds_nodes"] == 284 and c["lds_default_s7"]["lds_nodes"] == 298   # their TLAS sizes
    assert c["lds_nodes_off_s0"]["lds_nodes"] == 0 and c["lds_nodes_off_s7"]["lds_nodes"] == 0
    assert c["extra_features_all_s7"]["variant_features"] == 4095
    assert c["auto_s5"]["slab32"] == 0 and c["camera_far_s0"]["slab32"] == 0 and c["lds_default_s0"]["slab32"] == 1
    assert c["auto_s5_f32"]["slab32"] == 1 and c["auto_s0_f32"]["slab32"] == 1
    assert not any(v for k, v in c["empty_tile_shard_s0"].items() if k != "spp_chunk")
    for a, b in (("accum_pool_s0", "pool_inorder_s0"), ("accum_pool_s5", "pool_overlap_s5"),
                 ("accum_items_s5", "items_chunk_batches_s5")):
        assert c[a] == c[b]


def test_every_attempt_upholds_the_plans_invariants(attempts):
    """Each case at its own bound and at that bound halved down to 1 MiB, with the ring allowed
    and ruled out: every plan the out-of-memory loop can reach."""
    _, cases = golden()
    n = 0
    for c in cases:
        chunk = c["expect"]["spp_chunk"]
        bounds = {a["bound"] for a in attempts[c["case"]]}
        if c["expect"]["samples"]:   # (the empty shard is one all-zero plan)
            assert min(bounds) == MIB and max(bounds) == c["buf_bytes"], c["case"]
            assert all(sum(a["bound"] == b for a in attempts[c["case"]]) == 2 for b in bounds), c["case"]
        for a in attempts[c["case"]]:
            if not a["total"]:
                continue
            n += 1
            why = "%s at %d (ring allowed: %d)" % (c["case"], a["bound"], a["ring_allowed"])
            assert a["err"] == 0, why
            assert a["n_batches"] * a["batch"] >= a["total"] > (a["n_batches"] - 1) * a["batch"], why
            assert a["per_sample"] or a["batch"] % chunk == 0 or a["batch"] == a["total"], why
            assert not a["overlapped"] or (a["n_batches"] >= 2 and a["schedule"] != 0), why
            assert a["per_sample"] == (a["schedule"] == POOL and not a["ring"]), why
            assert not a["ring"] or (a["block_samples"] == chunk <= 16 and a["ring_allowed"]), why
            assert a["trace_buf_bytes"] == (2 if a["overlapped"] else 1) * a["half_bytes"] + a["ring_bytes"], why
    assert n > 4 * len(cases)


def test_a_camera_shutter_outside_the_scenes_time_range_is_refused(plan_dump, tmp_path):
    """A moving sphere's boxes bound it for the ray times the tables were built for (flatten.cpp's
    box invariant; [0, 1] unless RT_BUILD_TIME0 / _TIME1 say otherwise). The plan refuses a camera
    whose time0 / time1 leave that range, before anything is allocated or launched, on a scene that
    holds a moving sphere (the random scene) and on no other (the Cornell box)."""
    dev, _ = golden()
    frame = dict(width=64, height=48, spp=4)
    cases = {
        "inside": dict(scene=0, cam_time0=0.25, cam_time1=0.75),
        "equal": dict(scene=0, cam_time0=0.0, cam_time1=1.0),
        "reversed": dict(scene=0, cam_time0=1.0, cam_time1=0.0),
        "late": dict(scene=0, cam_time0=0.0, cam_time1=1.5),
        "early": dict(scene=0, cam_time0=-0.001, cam_time1=1.0),
        "disjoint": dict(scene=0, cam_time0=2.0, cam_time1=3.0),
        "built_for_it": dict(scene=0, cam_time0=-0.5, cam_time1=1.5, build_time0=-0.5, build_time1=1.5),
        "built_reversed": dict(scene=0, cam_time0=-0.5, cam_time1=1.5, build_time0=1.5, build_time1=-0.5),
        "built_narrower": dict(scene=0, cam_time0=0.0, cam_time1=1.0, build_time0=0.25, build_time1=0.75),
        "nothing_moves": dict(scene=5, cam_time0=-3.0, cam_time1=7.0),
    }
    path = tmp_path / "cases.json"
    path.write_text("\n".join([json.dumps(dev)] + [json.dumps(dict(DEFAULTS, case=k, **frame, **v)) for k, v in cases.items()]) + "\n")
    out = plan_dump(str(path))
    assert {a["case"] for a in out} == set(cases)
    refused = {"late", "early", "disjoint", "built_narrower"}
    for a in out:   # every attempt of the out-of-memory loop, not only the first
        if a["case"] in refused:
            assert a["err"] == -3 and "time range" in a["err_msg"] and a["n_batches"] == 0 and a["trace_buf_bytes"] == 0, a
        else:
            assert a["err"] == 0 and a["err_msg"] == "" and a["n_batches"] >= 1, a


def test_hidden_plan_fields_follow_the_stated_rules(plan_dump, attempts, tmp_path):
    """What rt_stats does not show, against values worked out by hand from the rules as
    launch_plan.cpp states them."""
    dev, _ = golden()
    frames = {   # random scene, default options
        # 320x200: 40 x 25 = 1,000 tiles, chunks of 16. Blocks of 16 samples stay while tiles x
        # ceil(spp / 16) is not below 160,000: 2,560 spp gives 1,000 x 160 = 160,000, not below; 2,544
        # spp gives 1,000 x 159 = 159,000, so blocks halve to 8, where 1,000 x 318 = 318,000 holds
        "bs_2560": dict(scene=0, width=320, height=200, spp=2560),
        "bs_2544": dict(scene=0, width=320, height=200, spp=2544),
        # C2's one-of-eight row shard, 1200x100x500: 150 x 13 = 1,950 tiles; blocks of 16: 1,950 x 32
        # = 62,400; of 8: 1,950 x 63 = 122,850; both below 160,000, and 4 is the floor
        "bs_c2_shard": dict(scene=0, width=1200, height=800, spp=500, row_stride=8),
    }
    path = tmp_path / "cases.json"
    path.write_text("\n".join([json.dumps(dev)] + [json.dumps(dict(DEFAULTS, case=k, **v)) for k, v in frames.items()]) + "\n")
    got = {a["case"]: a for a in plan_dump(str(path)) if a["primary"]}
    assert got["bs_2560"]["spp_chunk"] == 16 and got["bs_2544"]["spp_chunk"] == 16 and got["bs_c2_shard"]["spp_chunk"] == 16
    assert got["bs_2560"]["block_samples"] == 16
    assert got["bs_2544"]["block_samples"] == 8
    assert got["bs_c2_shard"]["samples"] == 1200 * 100 * 500 and got["bs_c2_shard"]["block_samples"] == 4

    def primary(name):
        return [a for a in attempts[name] if a["primary"]][0]
    # the final scene's 1024-thread workgroups stage "the whole BLAS" (RT_BLOCK_FINAL's comment)
    s7 = primary("lds_default_s7")
    assert s7["n_blas_bfs"] > 0 and s7["n_lds_blas"] == s7["n_blas_bfs"]
    # nothing is staged once rt_ctx_set_variant turns lds_nodes off; the random scene has no BLAS
    assert primary("lds_nodes_off_s7")["n_lds_blas"] == 0 and primary("lds_nodes_off_s7")["n_lds_materials"] == 0
    assert primary("lds_default_s0")["n_blas_bfs"] == 0 and primary("lds_default_s0")["n_lds_blas"] == 0
