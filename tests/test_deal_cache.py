"""The whole-frame deal order's cache (csrc/deal_cache.cpp: which render measures, which builds
the order, which reuses it) pinned on the CPU.

tests/deal_cache_main.cpp links deal_cache.cpp alone — nothing from HIP — and plays a script of
renders against one rtd::DealCache. It is built twice, plain and as its own program with ASan and
UBSan (the program itself is instrumented, so nothing is preloaded); every script runs on both and
their outputs must agree.
"""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust-ray-tracing-in-a-weekend_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
BASE = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SOURCES = [os.path.join(REPO, "tests", "deal_cache_main.cpp"), os.path.join(CSRC, "deal_cache.cpp")]
EMPTY, MEASURED, ORDERED = 0, 1, 2   # rtd::DealCache::State
OFF, AUTO, MEASURE_ONLY = 0, 1, 2    # RT_OPT_AUTO_DEAL_ORDER


@pytest.fixture(scope="module")
def play(tmp_path_factory):
    """play(lines) -> one dict per command, from the plain and the sanitized build alike."""
    d = tmp_path_factory.mktemp("deal_cache")
    exes = []
    for name, flags in (("plain", []), ("san", SAN)):
        exe = str(d / ("deal_cache_main_" + name))
        b = subprocess.run([CLANG, *BASE, *flags, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
        exes.append(exe)
    n = [0]

    def run(lines):
        n[0] += 1
        script = d / ("script%d.txt" % n[0])
        script.write_text("\n".join(lines) + "\n")
        outs = []
        for exe in exes:
            env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                       UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
            r = subprocess.run([exe, str(script)], capture_output=True, text=True, env=env, timeout=120)
            report = r.stdout + r.stderr
            assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
            assert r.returncode == 0, report[-4000:]
            outs.append(r.stdout)
        assert outs[0] == outs[1]
        got = [json.loads(line) for line in outs[0].splitlines()]
        assert len(got) == len(lines)
        return got
    return run


def render(mode=AUTO, kind="frame", gen=1, cam=0, w=156, h=92):
    return "render %d %s %d %g %d %d" % (mode, kind, gen, cam, w, h)


def what(r):
    return (r["measure"], r["build"], r["ordered"], r["state"])


MEASURE = (1, 0, 0, MEASURED)
BUILD = (0, 1, 1, ORDERED)
REUSE = (0, 0, 1, ORDERED)


def test_a_key_measures_then_builds_then_reuses(play):
    got = play([render()] * 5)
    assert [what(r) for r in got] == [MEASURE, BUILD, REUSE, REUSE, REUSE]
    assert all(r["eligible"] == 1 and r["n_tiles"] == 240 for r in got)
    assert sorted(got[1]["built"]) == list(range(240)) and got[4]["order_len"] == 240
    # the item pool is a pool schedule too
    assert [what(r) for r in play([render(kind="items")] * 3)] == [MEASURE, BUILD, REUSE]


@pytest.mark.parametrize("other", [dict(cam=1), dict(w=164), dict(h=100), dict(gen=2)])
def test_another_key_starts_over(play, other):
    got = play([render(), render(), render(), render(**other), render(**other), render(**other), render()])
    assert [what(r) for r in got] == [MEASURE, BUILD, REUSE, MEASURE, BUILD, REUSE, MEASURE]


def test_a_frame_of_as_many_tiles_is_still_another_key(play):
    # 156x92 and 160x96 are both 20 x 12 tiles
    got = play([render(), render(), render(w=160, h=96), render(w=160, h=96)])
    assert [what(r) for r in got] == [MEASURE, BUILD, MEASURE, BUILD]


def test_drop_forgets_the_entry(play):
    got = play([render(), render(), "drop", render(), render()])
    assert got[2]["state"] == EMPTY
    assert [what(got[i]) for i in (0, 1, 3, 4)] == [MEASURE, BUILD, MEASURE, BUILD]


@pytest.mark.parametrize("kind", ["tile_shard", "row_shard", "count", "chunks", "adaptive"])
def test_ineligible_renders_leave_the_entry_alone(play, kind):
    got = play([render(kind=kind), render(), render(kind=kind), render(kind=kind, cam=3), render(),
                render(kind=kind), render()])
    assert [r["eligible"] for r in got] == [0, 1, 0, 0, 1, 0, 1]
    assert [what(r) for r in got] == [(0, 0, 0, EMPTY), MEASURE, (0, 0, 0, MEASURED), (0, 0, 0, MEASURED), BUILD,
                                      (0, 0, 0, ORDERED), REUSE]


def test_option_off_decides_nothing_and_keeps_the_entry(play):
    got = play([render(OFF), render(), render(OFF), render(), render(OFF), render(OFF, cam=2), render()])
    assert [what(r) for r in got] == [(0, 0, 0, EMPTY), MEASURE, (0, 0, 0, MEASURED), BUILD, (0, 0, 0, ORDERED),
                                      (0, 0, 0, ORDERED), REUSE]


def test_measure_only_measures_every_render_and_never_orders(play):
    got = play([render(MEASURE_ONLY)] * 4 + [render(), render(), render(MEASURE_ONLY), render()])
    assert [what(r) for r in got[:4]] == [MEASURE] * 4
    # its last measurement serves the default mode; measuring again takes the order back
    assert [what(r) for r in got[4:]] == [BUILD, REUSE, MEASURE, BUILD]
    assert all(r["measure"] + r["ordered"] <= 1 for r in got)   # a render never measures what it reorders


def test_order_from_costs(play):
    n = 240
    equal, = play(["order " + " ".join(["7"] * n)])
    assert equal["order"] == list(range(n))   # equal costs: raster
    costs = [(i * 37) % 11 for i in range(n)]   # many ties, some zero (tiles with no measured block)
    got, = play(["order " + " ".join(map(str, costs))])
    o = got["order"]
    assert sorted(o) == list(range(n))
    assert all(costs[a] > costs[b] or (costs[a] == costs[b] and a < b) for a, b in zip(o, o[1:]))
    zeros = [i for i in range(n) if costs[i] == 0]
    assert zeros and o[-len(zeros):] == zeros   # unmeasured tiles last, in raster order
    assert play(["order"])[0]["order"] == []
    # the build uses the same order, on the costs read back
    built = play(["costs " + " ".join(map(str, costs)), render(), render()])[2]["built"]
    assert built == o
    big = play(["order %d 1 %d 0" % (2**64 - 1, 2**63)])[0]["order"]   # the full u64 range
    assert big == [0, 2, 1, 3]
