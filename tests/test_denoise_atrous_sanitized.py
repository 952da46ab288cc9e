"""rt_denoise_atrous_host under ASan and UBSan, built the way tests/test_denoise_sanitized.py builds
its program.

tests/atrous_host_main.cpp has its own main and links csrc/atrous_host.cpp alone (no HIP include
path, no HIP library). The program itself is instrumented and run directly: nothing is preloaded.
Every buffer — the frame, the map, the guides, both outputs — is exactly its frame's size, so a
read or write past an edge is reported. It prints two checksums per output and case (sum_i x_i and
sum_i c_i x_i, c_i = 1 + i mod 7); the same sums of the numpy reference
(tests/denoise_atrous_reference.py) must agree within sum_i c_i (1e-11 + 1e-11 |ref_i|), the
per-element tolerance summed.
"""
import os
import re
import struct
import subprocess

import numpy as np

from tests import denoise_atrous_reference as atr
from tests import denoise_reference as dr
from tests.test_denoise_sanitized import CLANG, CSRC, FLAGS, REPO, _frame

SOURCES = [os.path.join(REPO, "tests", "atrous_host_main.cpp"), os.path.join(CSRC, "atrous_host.cpp")]

#        W,  H,  dtype,      levels, demodulate, guide mask (1 albedo, 2 normal, 4 depth)
CASES = [(1, 1, np.float64, 3, 0, 0),
         (1, 1, np.float32, 1, 1, 7),
         (9, 5, np.float64, 6, 0, 7),          # every tap of steps >= 4 is outside
         (9, 5, np.float32, 6, 1, 1),
         (17, 16, np.float64, 3, 1, 7),
         (17, 16, np.float32, 5, 0, 0),
         (72, 9, np.float64, 6, 0, 5),         # a step-32 tap inside the frame
         (72, 9, np.float32, 6, 1, 7)]


def test_atrous_host_filter_is_clean_under_asan_and_ubsan(tmp_path):
    exe, data = str(tmp_path / "atrous_host_main"), str(tmp_path / "cases.bin")
    b = subprocess.run([CLANG, *FLAGS, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    frames = [_frame(W, H, dt, 31 + i) for i, (W, H, dt, *_rest) in enumerate(CASES)]
    guides = []
    with open(data, "wb") as f:
        f.write(struct.pack("<i", len(CASES)))
        for (W, H, dt, levels, dem, mask), (mean, se) in zip(CASES, frames):
            g = [x if mask >> i & 1 else None for i, x in enumerate(atr.coord_guides(H, W))]
            guides.append(g)
            f.write(struct.pack("<6i4d", W, H, 1 if dt == np.float64 else 0, levels, dem, mask, atr.SIGMA_L, *atr.SIGMAS))
            f.write(mean.tobytes())
            f.write(se.tobytes())
            for x in g:
                if x is not None:
                    f.write(np.ascontiguousarray(x, dtype=np.float64).tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    run = subprocess.run([exe, data], capture_output=True, text=True, env=env, timeout=120)
    report = run.stdout + run.stderr
    assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert run.returncode == 0, report[-4000:]
    sums = re.findall(r"^case (\d+) .* sum (\S+) weighted (\S+) se_sum (\S+) se_weighted (\S+)$", run.stdout, flags=re.M)
    assert [int(s[0]) for s in sums] == list(range(len(CASES))), run.stdout
    for (W, H, dt, levels, dem, mask), (mean, se), g, (_, s0, s1, e0, e1) in zip(CASES, frames, guides, sums):
        ref, se_ref = atr.atrous(mean, se, levels, atr.SIGMA_L, *g, atr.SIGMAS, bool(dem))
        for what, got0, got1, r, f32 in (("out", s0, s1, ref, dt == np.float32), ("stderr_out", e0, e1, se_ref, False)):
            r = r.astype(np.float64).reshape(-1)
            c = 1.0 + np.arange(r.size) % 7
            if f32:                  # one f32 ulp of each rounded reference value
                tol = np.spacing(np.abs(r).astype(np.float32)).astype(np.float64)
            else:
                tol = dr.TOL_ABS + dr.TOL_REL * np.abs(r)
            d0, d1 = abs(float(got0) - r.sum()), abs(float(got1) - (c * r).sum())
            print(f"{W}x{H} {np.dtype(dt).name} L={levels} demodulate {dem} guides {mask} {what}: |sum - ref| {d0:.3e} "
                  f"(bound {tol.sum():.3e}), weighted {d1:.3e} (bound {(c * tol).sum():.3e})")
            assert d0 <= tol.sum() and d1 <= (c * tol).sum()
