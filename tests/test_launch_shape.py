"""The kernel shape of a trace launch (csrc/launch_shapes.hpp: KernelShape, kernel_shape,
launch_shape, lds_layout) on the CPU.

tests/shape_dump.cpp includes the HIP-free headers only and is built with ASan and UBSan (the
program itself is instrumented, so nothing is preloaded). It resolves the shape of every variant
feature set x slab32 x lds_stack x f32 x {no TLAS in LDS, part of it, all of it} x stack16_ok as the
host does, and the rules are restated here independently of the header: which launches keep 16-bit
stack entries, the workgroup sizes, and a few LDS totals summed by hand.
"""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust-ray-tracing-in-a-weekend_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SPHERES, RECTINST, MEDIA, FINAL, ALL = 0, 35, 103, 287, 4095   # scene_features.hpp: FEAT_SET_*, FEAT_ALL
N_TLAS = 284   # the random scene's TLAS (shape_dump's enumeration uses it)


@pytest.fixture(scope="module")
def shape_dump(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shape_dump") / "shape_dump")
    b = subprocess.run([CLANG, *FLAGS, "-I" + os.path.join(REPO, "include"), "-I" + CSRC,
                        os.path.join(REPO, "tests", "shape_dump.cpp"), "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]

    def run(*args):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                   UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, env=env, timeout=60)
        report = r.stdout + r.stderr
        assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
        assert r.returncode == 0, report[-4000:]
        return [json.loads(line) for line in r.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def shapes(shape_dump):
    got = shape_dump()
    assert len(got) == 5 * 2 * 2 * 2 * 3 * 2
    assert {a["variant"] for a in got} == {SPHERES, RECTINST, MEDIA, FINAL, ALL}
    return got


def test_host_resolver_round_trips_through_the_template_coordinates(shapes):
    for a in shapes:
        assert a["round_trip"] == 1, a
        assert (a["features"], a["s32"], a["lds"], a["f32"]) == (a["variant"], a["slab32"], a["lds_stack"], a["prec_f32"]), a
        whole = a["n_lds_nodes"] == a["n_tlas_nodes"]
        # the whole TLAS staged is NALL, but for a spheres launch whose stack entries do not fit 16 bits
        narrow = a["stack16_switch"] and a["variant"] == SPHERES and a["slab32"] and a["lds_stack"]
        assert a["nall"] == int(whole and not (narrow and not a["stack16_ok"])), a
        # the two views of the shape (block_threads_of, stack16_launch: the latter is of a spheres launch)
        assert a["block_threads_of"] == a["block_threads"], a
        assert a["variant"] != SPHERES or a["stack16_launch"] == a["s16"], a
    assert {a["nall"] for a in shapes} == {0, 1}


def test_stack16_exactly_where_every_condition_holds(shapes):
    n = 0
    for a in shapes:
        want = (a["variant"] == SPHERES and a["slab32"] == 1 and a["lds_stack"] == 1 and
                a["n_lds_nodes"] == a["n_tlas_nodes"] == N_TLAS and a["stack16_ok"] == 1 and a["stack16_switch"] == 1)
        assert a["s16"] == int(want), a
        assert a["entry_bytes"] == (2 if want else 4), a
        assert a["node_bytes"] == (80 if a["nall"] and a["s32"] else 64), a
        n += want
    assert n == 2 * shapes[0]["stack16_switch"]   # f64 and f32


def test_workgroup_sizes(shapes):
    for a in shapes:
        if a["variant"] == FINAL:
            want = 1024
        elif a["s16"]:
            want = 512 if a["f32"] else 768
        else:
            want = 256
        assert a["block_threads"] == want, a
        assert a["stage_shade"] == int(a["variant"] != SPHERES), a
        assert a["stage_blas"] == int(a["variant"] in (FINAL, ALL)), a   # the feature sets with FEAT_INST_BLAS
        # the launch bounds (waves per SIMD): what launch_plan.cpp's 16, 12 and 24 waves per CU are four times
        assert a["min_waves"] == (4 if a["variant"] == FINAL else 6 if a["s16"] else 1 if a["variant"] == SPHERES else 3), a


def test_lds_totals_summed_by_hand(shape_dump):
    def layout(variant, slab32, lds, f32, n_lds, n_tlas, ok, n_blas, entries, n_mat, n_tex):
        return shape_dump(variant, slab32, lds, f32, n_lds, n_tlas, ok, n_blas, entries, n_mat, n_tex)[0]

    # the random scene, f64, 16-bit stack: 284 nodes x 80 B = 22,720 (22.2 KB), 13 entries x 768 lanes
    # x 2 B = 19,968 (19.5 KB), no tables staged whatever their size; then 32 B x 768 = 24,576 (24 KB) of seeds
    a = layout(SPHERES, 1, 1, 0, 284, 284, 1, 0, 13, 485, 485)
    if a["s16"]:
        assert (a["blas"], a["stack"], a["shade"], a["total"]) == (22720, 22720, 42688, 42688)
        assert a["seeds"] == 42688 and a["seed_stage_bytes"] == 24576 and a["seeds"] + a["seed_stage_bytes"] == 67264
        # 283 nodes: 22,640 + 19,968 = 42,608, and the slots start on the next 32 B boundary
        b = layout(SPHERES, 1, 1, 0, 283, 283, 1, 0, 13, 0, 0)
        assert b["total"] == 42608 and b["seeds"] == 42624
    # a final-scene launch: 100 x 80 + 597 BLAS nodes x 64 + 13 x 1024 x 4 + 10 x 64 + 12 x 96
    a = layout(FINAL, 1, 1, 0, 100, 100, 1, 597, 13, 10, 12)
    assert (a["blas"], a["stack"], a["shade"], a["total"]) == (8000, 46208, 99456, 8000 + 38208 + 53248 + 640 + 1152)
    assert a["total"] == 101248
    # spheres whose entries do not fit 16 bits: the partial-TLAS shape, 64 B nodes, 32-bit entries, 256 lanes
    a = layout(SPHERES, 1, 1, 0, 500, 500, 0, 0, 20, 0, 0)
    assert (a["s16"], a["nall"], a["block_threads"]) == (0, 0, 256) and a["total"] == 500 * 64 + 20 * 256 * 4 == 52480
    # the Cornell variant with f64 slabs and the scratch stack: no BLAS staged (no nested walk), no stack
    a = layout(RECTINST, 0, 0, 0, 10, 10, 1, 50, 20, 6, 5)
    assert (a["blas"], a["stack"], a["shade"], a["total"]) == (640, 640, 640, 640 + 6 * 64 + 5 * 96) and a["total"] == 1504
