"""rt_denoise_cross_host under ASan and UBSan, built the way tests/test_denoise_sanitized.py builds
its program.

tests/denoise_cross_host_main.cpp has its own main and links csrc/cross_host.cpp alone (no HIP
include path, no HIP library). The program itself is instrumented and run directly: nothing is
preloaded. Its buffers are exactly the frame's size, so an access past a frame's edge is reported. It
prints two checksums of out and two of stderr_out per case (sum_i v_i and sum_i c_i v_i, c_i = 1 +
i mod 7); the same sums of the numpy reference (tests/denoise_cross_reference.py) must agree within
sum_i c_i (1e-11 + 1e-11 |ref_i|), the per-element tolerance summed (f32 frames: one f32 ulp of each
rounded reference value).
"""
import os
import re
import struct
import subprocess

import numpy as np

from tests import denoise_cross_reference as cr
from tests import denoise_guided_reference as gr
from tests import denoise_reference as dr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust-ray-tracing-in-a-weekend_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-ffp-contract=off"]
SOURCES = [os.path.join(REPO, "tests", "denoise_cross_host_main.cpp"), os.path.join(CSRC, "cross_host.cpp")]

#        W,  H,  dtype,      radius, patch, k, guided
CASES = [(37, 21, np.float64, 3, 1, 0.45, False),
         (37, 21, np.float32, 10, 3, 0.45, True),
         (9, 5, np.float64, 5, 2, 1.0, True),      # the window is larger than the frame
         (1, 1, np.float64, 10, 3, 0.45, False),
         (1, 1, np.float32, 1, 0, 0.45, True)]


def _frame(W, H, dtype, seed):
    """A smooth ramp plus noise whose scale the error map states, drawn once per half at sqrt(2) of
    it; a fifth of the pixels noise-free."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    se = np.where(rng.random((H, W)) < 0.2, 0.0, 0.02 + 0.1 * rng.random((H, W)))
    base = (0.2 + 0.05 * x + 0.03 * y)[..., None] * np.array([1.0, 0.8, 0.6])
    a = base + np.sqrt(2.0) * se[..., None] * rng.standard_normal((H, W, 3))
    b = base + np.sqrt(2.0) * se[..., None] * rng.standard_normal((H, W, 3))
    return a.astype(dtype), b.astype(dtype), se


def _tol(ref, f32):
    if f32:     # one f32 ulp of each rounded reference value
        return np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return dr.TOL_ABS + dr.TOL_REL * np.abs(ref)


def test_host_cross_filter_is_clean_under_asan_and_ubsan(tmp_path):
    exe, data = str(tmp_path / "denoise_cross_host_main"), str(tmp_path / "cases.bin")
    b = subprocess.run([CLANG, *FLAGS, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    frames = [_frame(W, H, dt, 23 + i) for i, (W, H, dt, *_rest) in enumerate(CASES)]
    guides = [gr.cpu_guides(0.5 * (fa.astype(np.float64) + fb), seed=7 + i) if c[6] else None
              for i, (c, (fa, fb, _)) in enumerate(zip(CASES, frames))]
    with open(data, "wb") as f:
        f.write(struct.pack("<i", len(CASES)))
        for (W, H, dt, r, p, k, guided), (ma, mb, se), g in zip(CASES, frames, guides):
            f.write(struct.pack("<6i2d", W, H, 1 if dt == np.float64 else 0, r, p, int(guided), k, cr.SCALE))
            for arr in (ma, mb, se):
                f.write(arr.tobytes())
            if guided:
                for arr in g:
                    f.write(np.ascontiguousarray(arr, dtype=np.float64).tobytes())
                f.write(struct.pack("<3d", *gr.SIGMAS))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe, data], capture_output=True, text=True, env=env, timeout=120)
    report = run.stdout + run.stderr
    assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert run.returncode == 0, report[-4000:]
    sums = re.findall(r"^case (\d+) .* sum (\S+) weighted (\S+) stderr (\S+) weighted (\S+)$", run.stdout, flags=re.M)
    assert [int(s[0]) for s in sums] == list(range(len(CASES))), run.stdout
    for (W, H, dt, r, p, k, guided), (ma, mb, se), g, (_, s0, s1, e0, e1) in zip(CASES, frames, guides, sums):
        kw = dict(albedo=g[0], normal=g[1], depth=g[2], sigmas=gr.SIGMAS) if guided else {}
        ref, ref_se = cr.denoise_cross(ma, mb, se, r, p, k, cr.SCALE, **kw)
        for what, v, (g0, g1), f32 in (("out", ref.astype(np.float64).reshape(-1), (s0, s1), dt == np.float32),
                                       ("stderr_out", ref_se.reshape(-1), (e0, e1), False)):
            c = 1.0 + np.arange(v.size) % 7
            tol = _tol(v, f32)
            d0, d1 = abs(float(g0) - v.sum()), abs(float(g1) - (c * v).sum())
            print(f"{W}x{H} {np.dtype(dt).name} r={r} f={p} {what}: |sum - ref| {d0:.3e} (bound {tol.sum():.3e}), "
                  f"weighted {d1:.3e} (bound {(c * tol).sum():.3e})")
            assert d0 <= tol.sum() and d1 <= (c * tol).sum()
