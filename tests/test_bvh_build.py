"""The BVH builder (csrc/bvh_build.cpp: the SAH build, the LINEAR / MEDIAN chain, the f32 node
boxes, the stack a walk needs) on its own, on the CPU.

tests/bvh_build_main.cpp links bvh_build.cpp alone — no World, nothing from HIP — and builds over
the smallest sets of boxes at which each rule can go wrong. It is compiled as tests/test_lowering.py
compiles lower_dump, with ASan and UBSan (the program itself is instrumented, so nothing is
preloaded). The expected values are the rules as csrc/bvh_build.hpp states them with its defaults
(force_leaf 2, root_leaf 8, leaves of at most 31, the kernel's 32 stack entries), not the
program's output.
"""
import json
import os
import subprocess

import pytest

from tests.test_lowering import CLANG, CSRC, FLAGS, REPO

SOURCES = [os.path.join(REPO, "tests", "bvh_build_main.cpp"), os.path.join(CSRC, "bvh_build.cpp")]
EMPTY_LEAF = ~0   # RT_LEAF_CODE(0, 0)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bvh_build") / "bvh_build_main")
    b = subprocess.run([CLANG, *FLAGS, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert r.returncode == 0, report[-4000:]
    return {c["case"]: c for c in map(json.loads, r.stdout.splitlines())}


def test_sah_leaf_rules(cases):
    assert cases["sah_0"]["root"] == EMPTY_LEAF and cases["sah_0"]["n_nodes"] == 0 and cases["sah_0"]["n_prim_refs"] == 0
    # one item; force_leaf (with root_leaf 0, so that it decides); root_leaf, which comes before the pair rules
    for name, n in (("sah_1", 1), ("sah_2_plain", 2), ("sah_8", 8), ("sah_2_costly_whole_bvh", 2)):
        assert (cases[name]["root_leaf_count"], cases[name]["n_nodes"], cases[name]["need"]) == (n, 0, 0), name
    for name in ("sah_2_costly", "sah_2_in_blas"):   # a costly test, or a BLAS: the cost model splits a pair (root_leaf 0)
        assert (cases[name]["root"], cases[name]["n_nodes"], cases[name]["need"]) == (0, 1, 1), name
    assert cases["sah_9"]["root"] == 0 and cases["sah_9"]["n_nodes"] >= 1
    assert cases["sah_100"]["n_nodes"] >= 100 // 31   # no leaf can hold more


def test_sah_depth_cap_keeps_concentric_shells_within_the_kernels_stack(cases):
    c = cases["sah_concentric_200"]
    assert 21 < c["need"] + 1 <= 32   # past the depth the median split starts at, within the stack


def test_chain_keeps_list_order(cases):
    assert cases["chain_0"]["root"] == EMPTY_LEAF and cases["chain_0"]["chain_nodes"] == 0
    assert cases["chain_31"]["root_leaf_count"] == 31 and cases["chain_31"]["chain_nodes"] == 0
    c = cases["chain_32"]
    assert (c["chain_nodes"], c["segments"], c["unbounded"], c["need"]) == (1, ["leaf:31", "leaf:1"], True, 1)
    s = cases["chain_subtree"]
    assert s["chain_nodes"] == 2 and s["unbounded"]
    assert s["segments"][0] == "leaf:3" and s["segments"][1].startswith("node:") and s["segments"][2] == "leaf:2"
    assert int(s["segments"][1][5:]) < s["n_nodes"] - s["chain_nodes"]   # the subtree's root, built before the chain


def test_every_tree_holds_each_prim_once_in_leaves_of_at_most_31_inside_its_boxes(cases):
    trees = [c for c in cases.values() if "prims_once" in c]
    assert len(trees) == 14
    for c in trees:
        assert c["prims_once"] and c["max_leaf"] <= 31 and c["contained"], c["case"]


def test_stack_need_rule_cycle_and_shared_memo(cases):
    c = cases["stack_rule"]
    assert c["leaf"] == 0
    # children needing n0, n1: 1 + max(n0, n1); with bit-identical child boxes max(1 + n0, n1)
    want = {"differ_1_2": 3, "differ_2_1": 3, "same_1_2": 2, "same_2_1": 3, "same_0_0": 1, "differ_0_0": 1}
    for name, need in want.items():
        assert c[name] == need and c[name + "_again"] == need, name
    assert c["appended"] == 4 and c["cycle"] == -1


def test_renumbering_puts_the_tlas_first_and_visits_a_twice_named_child_once(cases):
    r = cases["renumber"]
    # root 1 -> 0, its one child 2 -> 1 (named twice, counted once), the BLAS node 0 -> 2; an instance over a
    # primitive keeps its child; a leaf root leaves everything alone
    assert (r["n_tlas_nodes"], r["root"], r["n_nodes"], r["root_children"]) == (2, 0, 3, [1, 1])
    assert r["blas_root"] == 2 and r["prim_child"] == 0 and r["leaf_root"] == 1


def test_build_option_clamps(cases):
    p = cases["params"]
    assert p["default"] == [1, 8, 2, 8, 1, 1]
    assert p["clamped"] == [0.01, 2, 31, 31, 0, 1]
