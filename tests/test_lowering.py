"""The host lowering (csrc/scene_lower.cpp: validation, device tables, stack sizes, feature bits)
pinned on the CPU.

tests/lower_dump.cpp links the scene builders, the flattener and the lowering — nothing from
HIP — and prints one JSON line per scene: the eight reference scenes, the small worlds of
tests/test_gpu_nesting.py and a few tables no flattener produces. It is built with ASan and
UBSan (the program itself is instrumented, so nothing is preloaded) and its output must equal
tests/golden/lowering.json, which was produced by the upload code as it stood in abi.cpp
before the lowering became a module of its own.

    python -m tests.test_lowering      regenerates the golden file (only when the lowering is
                                       meant to change; review the diff)
"""
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust-ray-tracing-in-a-weekend_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "lowering.json")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-ffp-contract=off"]
# the HIP-free sources from the scene builders to the lowering (tests/test_launch_plan.py and
# tests/test_seed_stage_plan.py link them too)
LOWERING_SOURCES = [os.path.join(CSRC, f) for f in ("scene_model.cpp", "flatten.cpp", "bvh_build.cpp", "scene_lower.cpp")]
SOURCES = [os.path.join(REPO, "tests", "lower_dump.cpp")] + LOWERING_SOURCES


def run_dump(workdir: str) -> str:
    """Builds lower_dump in workdir (no HIP include path, no HIP library) and returns its output."""
    exe = os.path.join(workdir, "lower_dump")
    b = subprocess.run([CLANG, *FLAGS, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert r.returncode == 0, report[-4000:]
    return r.stdout


def test_lowering_matches_golden_under_asan_and_ubsan(tmp_path):
    got = [json.loads(line) for line in run_dump(str(tmp_path)).splitlines()]
    want = [json.loads(line) for line in open(GOLDEN)]
    assert [g["case"] for g in got] == [w["case"] for w in want]
    for g, w in zip(got, want):
        assert g == w, "%s: %s" % (g["case"], {k: (g.get(k), w.get(k)) for k in set(g) | set(w) if g.get(k) != w.get(k)})


def test_golden_agrees_with_what_the_project_states():
    """The figures the documents and the GPU tests quote, read from the golden file itself."""
    c = {w["case"]: w for w in map(json.loads, open(GOLDEN))}
    refused = {"refused_nonprimitive": "an instance BVH holds a non-primitive", "refused_cycle": "cycle in an instance BVH",
               "refused_nonprimitive_then_cycle": "an instance BVH holds a non-primitive", "refused_bad_node": "bad node"}
    # refused by the flattener itself, in every accel mode: an rt_world_bvh node over children the
    # reference's boxes do not bound (flatten.cpp's box invariant); the message names node and child
    at_flatten = ["unbounded_by_reference_under_bvh_" + a for a in ("sah", "linear", "median")]
    for name in at_flatten:
        w = c.pop(name)
        assert w["flatten_rc"] == -3 and w["err"].startswith("rt_world_bvh node ") and " its child " in w["err"], name
    # ... and lowered with the product's own boxes everywhere else (nodes only under SAH)
    assert c["unbounded_by_reference_sah"]["n_tlas_nodes"] > 0 and c["unbounded_by_reference_times_m1_4"]["n_tlas_nodes"] > 0
    for name, w in c.items():   # validate's refusals carry the messages tests/test_abi.py asserts on
        assert (w["rc"] != 0 and w["err"] == refused[name]) if name in refused else w["rc"] == 0, name
    # random scene: the spheres variant with 16-bit stack entries, its ground sphere hoisted
    assert c["scene0_sah"]["variant"] == 0 and c["scene0_sah"]["stack16_ok"] == 1
    assert c["scene0_sah"]["pre_leaf"] != 0 and c["scene0_sah_nohoist"]["pre_leaf"] == 0
    assert c["scene5_sah"]["features"] == 35 and c["scene6_sah"]["features"] == 103      # FEAT_SET_RECTINST, _MEDIA
    # final scene: its one deferred BLAS walk needs max(TLAS, BLAS) entries, and the BLAS is relocated
    f = c["scene7_sah"]
    assert f["variant"] == 287 and f["stack_entries"] == max(f["tlas_depth"], f["blas_depth"]) + 1
    assert f["n_blas_bfs"] > 0 and f["n_tlas_nodes"] + f["n_blas_bfs"] == f["n_nodes"]
    # tests/test_gpu_nesting.py's variants
    assert c["nested_sah"]["variant"] == 4095
    assert [c["shutter_%d" % i]["variant"] for i in range(3)] == [0, 4095, 4095]
    assert c["instanced_static"]["variant"] == 287 and c["instanced_moving"]["variant"] == 4095
    assert c["shared_blas_3"]["variant"] == 287 and c["shared_blas_40"]["variant"] == 287
    # a shared BLAS keeps one base; a second BLAS, or a second visit of one instance's slot, nests a walk
    assert c["shared_root_40"]["inst_pad"] == [40, 40] and c["shared_subtree_1"]["inst_pad"] == [0, 0]
    for name in ("two_blases", "instance_slot_twice"):
        assert c[name]["stack_entries"] == c[name]["tlas_depth"] + c[name]["blas_depth"] + 2
    once = c["instance_slot_once"]
    assert once["stack_entries"] == max(once["tlas_depth"], once["blas_depth"]) + 1
    assert c["image_rect"]["features"] & 2048 and c["image_instanced_sphere"]["features"] & 2048
    assert not c["image_top_sphere"]["features"] & 2048
    # no relative codes: Stack16 is decided by (n_prim_refs << 5) | 31
    assert c["instance_over_tlas_small"]["stack16_ok"] == 1 and c["instance_over_tlas_1023"]["stack16_ok"] == 0
    assert c["instance_beside_tlas_1023"]["stack16_ok"] == 1
    assert [c["sphere_field_%d" % n]["stack16_ok"] for n in (300, 613, 614, 1100)] == [1, 1, 0, 0]
    assert c["sphere_field_leaf31_1038"]["stack16_ok"] == 1 and c["sphere_field_leaf31_1039"]["stack16_ok"] == 0
    # a stack need of n takes n node levels, so above 21 the SAH build recursed past depth 20, where
    # its median split (bvh_build.cpp) is what keeps the walk within the kernel's 32 entries
    assert 21 < c["concentric_200"]["tlas_depth"] <= 32


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        open(GOLDEN, "w").write(run_dump(d))
    print("wrote", GOLDEN)
    sys.exit(0)
