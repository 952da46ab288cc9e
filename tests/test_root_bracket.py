"""The f32 root brackets of RT_OPT_DEFER_ROOTS (csrc/root_bracket.hpp) on the CPU.

The CfgDefer kernels decide a sphere test's three questions — near or far root against t_min, in
range or not, closer than the best so far or not — from f32 brackets of the f64 roots, and compute
the exact root of a cast's winner only. tests/root_bracket_main.cpp runs the header the kernel runs:

- containment: on more than 1e6 random inputs and the constructed edge cases (disc 0 / one ulp /
  1e-300, r = 1000 and 1e-3, origins on the surface, |d|^2 from 2^-60 to 2^60 and outside div_rcp's
  guard, infinite and NaN direction components) a bracket either holds sphere_t's computed f64 root
  strictly or the input is reported outside the bound's premises; everyday inputs never are;
- equivalence: a host twin of the deferred closest-hit loop returns the (slot, t bits) of the
  sequential exact loop (sphere_t with a shrinking t_max) in forward, reverse and 20 shuffled test
  orders: scene 0's spheres with bounce-like rays, identical spheres (the later-tested one wins),
  centres 1 ulp, 1e-12 and 1e-7 apart, rays that meet NaN;
- fallback share: on the scene-0 rays at most 1 % of the tests with disc >= 0 take the exact path
  (a bracket so wide that everything fell back would pass the rest and gain nothing);

and the same program is clean under ASan and UBSan.
"""
import json
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust-ray-tracing-in-a-weekend_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
MAIN_SOURCES = [os.path.join(REPO, "tests", "root_bracket_main.cpp")] + \
    [os.path.join(CSRC, f) for f in ("scene_model.cpp", "flatten.cpp", "bvh_build.cpp", "scene_lower.cpp")]


def _build_main(exe, flags):
    b = subprocess.run([CLANG, "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(REPO, "include"), "-I" + CSRC,
                        *MAIN_SOURCES, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]


def _check(d, min_inputs, min_scene_tests):
    # containment
    assert d["violations"] == 0
    assert d["inputs"] >= min_inputs and d["valid"] + d["ambiguous"] == d["inputs"]
    assert d["valid"] > d["inputs"] // 2 and d["ambiguous"] > 0          # both outcomes are exercised
    assert d["plain"] > 0 and d["plain_valid"] == d["plain"]             # |d|^2 ~ 1, scene-sized spheres: always in the premises
    assert d["worst"] < 1.0
    # equivalence
    assert d["mismatches"] == 0
    assert d["casts"] == 22 * d["rays"] and 0 < d["hits"] < d["casts"]
    assert d["other_exact"] > 0                                          # the coincident worlds do take the exact path
    # fallback share, on the scene-0 rays
    assert d["scene_tests"] >= min_scene_tests
    assert d["scene_exact"] * 100 <= d["scene_tests"]


def test_brackets_hold_and_the_deferred_loop_is_the_exact_loop(tmp_path):
    exe = str(tmp_path / "root_bracket_main")
    _build_main(exe, ["-O2"])
    r = subprocess.run([exe, "1000000", "1000"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(r.stdout)
    print(d)
    print("scene-0 tests with disc >= 0: %d, decided exactly: %d (%.3f %%)"
          % (d["scene_tests"], d["scene_exact"], 100.0 * d["scene_exact"] / d["scene_tests"]))
    _check(d, 1000000, 40000)


def test_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    """The program itself is instrumented and run directly (nothing is preloaded)."""
    exe = str(tmp_path / "root_bracket_main_san")
    _build_main(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe, "200000", "100"], capture_output=True, text=True, env=env, timeout=300)
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert r.returncode == 0, report[-4000:]
    _check(json.loads(r.stdout), 200000, 4000)
