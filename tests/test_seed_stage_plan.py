"""The host's decision about the wave-wide sample starts (rtp::Plan.seed_stage_bytes,
csrc/launch_plan.cpp; csrc/launch_shapes.hpp RT_STAGE_SEEDS) on the CPU.

tests/seed_stage_dump.cpp links the scene builders, the flattener, the lowering and the plan —
nothing from HIP — and prints the decision for each case of a case file. The rule, restated here
independently of launch_plan.cpp: the per-sample pool (buffer or ring) of the f64 spheres variant
in its 16-bit-stack configuration stages 32 B x 64 lanes x the workgroup's waves; every other
launch stages nothing; and staging is dropped when the LDS it adds would leave fewer workgroups
resident on a CU (allocations in 1 KB granules, at most 24 waves per CU).
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
BASE = ["-std=c++17", "-O1", "-g", "-ffp-contract=off"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SOURCES = [os.path.join(REPO, "tests", "seed_stage_dump.cpp")] + LOWERING_SOURCES + [os.path.join(CSRC, "launch_plan.cpp")]
POOL, ITEMS, CHUNKS = 1, 2, 0
SPHERES = 0            # rtk::FEAT_SET_SPHERES
WG_THREADS = 768       # RT_BLOCK_SPHERES: the f64 spheres variant's 16-bit-stack workgroup, 12 waves
STAGE = 32 * 64 * (WG_THREADS // 64)   # 24,576 B
KIB = 1024


def _build(tmp, flags, name):
    exe = str(tmp / name)
    b = subprocess.run([CLANG, *BASE, *flags, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
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
def dump(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("seed_stage_dump"), [], "seed_stage_dump")


def _staged_kernel(a):
    """The launch runs a kernel with a staged instantiation (restated from the issue, not from the plan)."""
    return (a["variant_features"] == SPHERES and a["precision"] == 0 and a["schedule"] == POOL and a["slab32"] == 1 and
            a["lds_stack"] == 1 and a["lds_nodes"] == a["n_tlas_nodes"] > 0 and a["stack16_ok"] == 1)


def _resident(lds_bytes, dev):
    """Workgroups of 12 waves resident on a CU: 24 waves per CU (6 per SIMD), LDS in 1 KB granules."""
    alloc = -(-lds_bytes // KIB) * KIB
    return 0 if alloc > dev["lds_per_block"] else min(24 // (WG_THREADS // 64), dev["lds_per_cu"] // alloc)


def test_staging_bytes_of_every_golden_case(dump):
    """The golden file's cases (every variant, schedule, precision and option the plan is pinned on):
    32 x 64 x waves per workgroup on the staged kernels, 0 on all others."""
    dev = json.loads(open(GOLDEN).readline())
    got = dump(GOLDEN)
    assert len(got) > 30 and all(a["err"] == 0 and a["slot_bytes"] == 32 for a in got)
    if not got[0]["switch"]:   # RT_STAGE_SEEDS 0: nothing stages
        assert not any(a["seed_stage_bytes"] for a in got)
        return
    n = 0
    for a in got:
        if _staged_kernel(a):
            assert a["stack16_launch"] == 1 and a["block_threads"] == WG_THREADS, a["case"]
            # the random scene: 284 nodes x 80 B + 2 B x 768 lanes x stack entries, two workgroups either way
            base = 80 * a["lds_nodes"] + 2 * WG_THREADS * a["stack_entries"]
            assert _resident(base + STAGE, dev) == _resident(base, dev) == 2, a["case"]
            assert a["seed_stage_bytes"] == STAGE == 24576, a["case"]
            n += 1
        else:
            assert a["seed_stage_bytes"] == 0, a["case"]
    assert n >= 5
    kinds = {(a["variant_features"], a["precision"], a["schedule"]) for a in got if not a["seed_stage_bytes"]}
    # none of: the spheres variant's item pool and f32 mode; the other variants' per-sample pools
    assert {(SPHERES, 0, ITEMS), (SPHERES, 1, POOL)} <= kinds
    assert len({v for v, _, s in kinds if v != SPHERES and s == POOL}) >= 3
    # both forms of the per-sample pool stage
    assert {a["ring"] for a in got if a["seed_stage_bytes"]} == {0, 1}


def test_staging_follows_the_kernel_the_launch_runs(dump, tmp_path):
    """The random scene, one option at a time: the launches that leave the staged kernels stage nothing."""
    dev = json.loads(open(GOLDEN).readline())
    cases = {   # name: (case keys, staged)
        "pool": ({}, True),
        "pool_ring": (dict(ring=2, spp_chunk=16, block_samples=16), True),
        "pool_count_work": (dict(count_work=1), True),
        "pool_accum": (dict(accum=1, spp_chunk=4), True),
        "pool_tile_shard": (dict(tile_shard=1, row_begin=1, row_stride=3), True),
        "chunks": (dict(sched=CHUNKS), False),
        "items": (dict(sched=ITEMS), False),
        "f32": (dict(prec=1), False),
        "f64_slabs": (dict(opt_slab32=0), False),
        "camera_far": (dict(cam_far=1), False),          # f64 slabs again
        "scratch_stack": (dict(opt_lds_stack=0), False),
        "no_lds_nodes": (dict(opt_lds_nodes=0), False),  # the partial-TLAS instantiation
        "all_features": (dict(extra_features=4095), False),
    }
    got = {a["case"]: a for a in dump(_cases(tmp_path, dev, {k: v for k, (v, _) in cases.items()}))}
    assert list(got) == list(cases)
    on = got["pool"]["switch"]
    assert got["pool_ring"]["ring"] == 1 and got["pool"]["ring"] == 0
    for k, (_, staged) in cases.items():
        assert got[k]["err"] == 0 and _staged_kernel(got[k]) == staged, k
        assert got[k]["seed_stage_bytes"] == (STAGE if staged and on else 0), k


def _cases(tmp_path, dev, cases):
    path = tmp_path / "cases.json"
    path.write_text("\n".join([json.dumps(dev)] + [json.dumps(dict(dict(case=k, scene=0, sched=POOL), **v)) for k, v in cases.items()]) + "\n")
    return str(path)


def test_staging_is_dropped_when_it_would_cost_a_resident_workgroup(dump, tmp_path):
    """The random scene (284 TLAS nodes: 22,720 B of records) with deeper stacks than its own, on the
    MI355X's 160 KB per CU. A workgroup's LDS without the slots is 22,720 + 1,536 x entries:
      22 entries: 56,512 B; with 24,576 B of slots 81,088 -> 80 KB granules: two workgroups, staged
      23 entries: 58,048 B (57 KB: two); with the slots 82,624 -> 81 KB: one workgroup: dropped
      36 entries: 78,016 B (77 KB: two); with the slots 102,592: one: dropped
      37 entries: 79,552 B (78 KB: two); with the slots 104,128: one: dropped
      40 entries: 84,160 B (83 KB: one already); with the slots 108,736 (107 KB): still one: staged
    and on a device with 64 KB of LDS the scene's own 42,688 B (13 entries) + slots do not fit a workgroup."""
    dev = json.loads(open(GOLDEN).readline())
    assert dev["lds_per_cu"] == 160 * KIB
    got = {a["case"]: a for a in dump(_cases(tmp_path, dev, {"e%d" % e: dict(stack_entries=e) for e in (22, 23, 36, 37, 40)}))}
    assert all(_staged_kernel(a) for a in got.values())
    if not got["e22"]["switch"]:   # RT_STAGE_SEEDS 0: nothing stages
        assert not any(a["seed_stage_bytes"] for a in got.values())
        return
    assert {k: a["seed_stage_bytes"] for k, a in got.items()} == {"e22": STAGE, "e23": 0, "e36": 0, "e37": 0, "e40": STAGE}
    small = dict(dev, lds_per_cu=64 * KIB, lds_per_block=64 * KIB)
    own = dump(_cases(tmp_path, small, {"own": {}}))[0]
    assert _staged_kernel(own) and 80 * own["lds_nodes"] + 2 * WG_THREADS * own["stack_entries"] == 42688
    assert own["seed_stage_bytes"] == 0


def test_dump_runs_clean_under_asan_and_ubsan(tmp_path):
    """The same program instrumented (nothing is preloaded: it is a stand-alone executable), once over the golden cases."""
    run = _build(tmp_path, SAN, "seed_stage_dump_san")
    assert len(run(GOLDEN)) > 30
