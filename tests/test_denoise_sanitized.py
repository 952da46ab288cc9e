"""rt_denoise_host under ASan and UBSan, built the way tests/test_lowering.py builds its program.

tests/denoise_host_main.cpp has its own main and links csrc/denoise_host.cpp alone (no HIP include
path, no HIP library). The program itself is instrumented and run directly: nothing is preloaded.
Its output buffers are exactly the frame's size, so a write past a frame's edge is reported. It
prints two checksums per case (sum_i out_i and sum_i c_i out_i, c_i = 1 + i mod 7); the same sums of
the numpy reference (tests/denoise_reference.py) must agree within sum_i c_i (1e-11 + 1e-11 |ref_i|),
the per-element tolerance summed.
"""
import os
import re
import struct
import subprocess

import numpy as np

from tests import denoise_reference as dr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust-ray-tracing-in-a-weekend_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-ffp-contract=off"]
SOURCES = [os.path.join(REPO, "tests", "denoise_host_main.cpp"), os.path.join(CSRC, "denoise_host.cpp")]

#        W,  H, dtype,      radius, patch, k
CASES = [(9, 5, np.float64, 10, 3, 0.45),      # the window is larger than the frame
         (1, 1, np.float64, 10, 3, 0.45),
         (1, 1, np.float32, 1, 0, 0.45),
         (17, 16, np.float64, 3, 1, 0.45),
         (17, 16, np.float32, 5, 2, 1.0)]


def _frame(W, H, dtype, seed):
    """A smooth ramp plus noise whose scale the error map states; a fifth of the pixels noise-free."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    se = np.where(rng.random((H, W)) < 0.2, 0.0, 0.02 + 0.1 * rng.random((H, W)))
    base = 0.2 + 0.05 * x + 0.03 * y
    mean = base[..., None] * np.array([1.0, 0.8, 0.6]) + se[..., None] * rng.standard_normal((H, W, 3))
    return mean.astype(dtype), se


def test_host_filter_is_clean_under_asan_and_ubsan(tmp_path):
    exe, data = str(tmp_path / "denoise_host_main"), str(tmp_path / "cases.bin")
    b = subprocess.run([CLANG, *FLAGS, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    frames = [_frame(W, H, dt, 11 + i) for i, (W, H, dt, *_rest) in enumerate(CASES)]
    with open(data, "wb") as f:
        f.write(struct.pack("<i", len(CASES)))
        for (W, H, dt, r, p, k), (mean, se) in zip(CASES, frames):
            f.write(struct.pack("<5id", W, H, 1 if dt == np.float64 else 0, r, p, k))
            f.write(mean.tobytes())
            f.write(se.tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe, data], capture_output=True, text=True, env=env, timeout=120)
    report = run.stdout + run.stderr
    assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert run.returncode == 0, report[-4000:]
    sums = re.findall(r"^case (\d+) .* sum (\S+) weighted (\S+)$", run.stdout, flags=re.M)
    assert [int(s[0]) for s in sums] == list(range(len(CASES))), run.stdout
    for (W, H, dt, r, p, k), (mean, se), (_, s0, s1) in zip(CASES, frames, sums):
        ref = dr.denoise(mean, se, r, p, k).astype(np.float64).reshape(-1)
        c = 1.0 + np.arange(ref.size) % 7
        if dt == np.float32:     # one f32 ulp of each rounded reference value
            tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        else:
            tol = dr.TOL_ABS + dr.TOL_REL * np.abs(ref)
        d0, d1 = abs(float(s0) - ref.sum()), abs(float(s1) - (c * ref).sum())
        print(f"{W}x{H} {np.dtype(dt).name} r={r} f={p}: |sum - ref| {d0:.3e} (bound {tol.sum():.3e}), "
              f"weighted {d1:.3e} (bound {(c * tol).sum():.3e})")
        assert d0 <= tol.sum() and d1 <= (c * tol).sum()
