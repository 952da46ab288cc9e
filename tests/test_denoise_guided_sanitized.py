"""rt_denoise_guided_host under ASan and UBSan, built the way tests/test_denoise_sanitized.py
builds its program.

tests/denoise_guided_host_main.cpp has its own main and links csrc/denoise_host.cpp alone (no HIP
include path, no HIP library). The program itself is instrumented and run directly: nothing is
preloaded. Every buffer — the frame, the map, the guides, the output — is exactly its frame's size,
so a read or write past an edge is reported. It prints two checksums per case (sum_i out_i and
sum_i c_i out_i, c_i = 1 + i mod 7); the same sums of the numpy reference
(tests/denoise_guided_reference.py) must agree within sum_i c_i (1e-11 + 1e-11 |ref_i|), the
per-element tolerance summed.
"""
import os
import re
import struct
import subprocess

import numpy as np

from tests import denoise_guided_reference as gr
from tests import denoise_reference as dr
from tests.test_denoise_sanitized import CLANG, CSRC, FLAGS, REPO, _frame

SOURCES = [os.path.join(REPO, "tests", "denoise_guided_host_main.cpp"), os.path.join(CSRC, "denoise_host.cpp")]

#        W,  H,  dtype,      radius, patch, k, guide mask (1 albedo, 2 normal, 4 depth)
CASES = [(37, 21, np.float64, 3, 1, 0.45, 7),
         (37, 21, np.float32, 10, 3, 0.45, 7),     # the window reaches past the frame on every side
         (9, 5, np.float64, 5, 2, 1.0, 5),
         (1, 1, np.float64, 1, 0, 0.45, 7)]


def test_guided_host_filter_is_clean_under_asan_and_ubsan(tmp_path):
    exe, data = str(tmp_path / "denoise_guided_host_main"), str(tmp_path / "cases.bin")
    b = subprocess.run([CLANG, *FLAGS, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    frames = [_frame(W, H, dt, 23 + i) for i, (W, H, dt, *_rest) in enumerate(CASES)]
    guides = []
    with open(data, "wb") as f:
        f.write(struct.pack("<i", len(CASES)))
        for (W, H, dt, r, p, k, mask), (mean, se) in zip(CASES, frames):
            g = [x if mask >> i & 1 else None for i, x in enumerate(gr.cpu_guides(mean, seed=W + H))]
            guides.append(g)
            f.write(struct.pack("<6i4d", W, H, 1 if dt == np.float64 else 0, r, p, mask, k, *gr.SIGMAS))
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
    sums = re.findall(r"^case (\d+) .* sum (\S+) weighted (\S+)$", run.stdout, flags=re.M)
    assert [int(s[0]) for s in sums] == list(range(len(CASES))), run.stdout
    for (W, H, dt, r, p, k, mask), (mean, se), g, (_, s0, s1) in zip(CASES, frames, guides, sums):
        ref = gr.denoise_guided(mean, se, r, p, k, *g, gr.SIGMAS).astype(np.float64).reshape(-1)
        c = 1.0 + np.arange(ref.size) % 7
        if dt == np.float32:     # one f32 ulp of each rounded reference value
            tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        else:
            tol = dr.TOL_ABS + dr.TOL_REL * np.abs(ref)
        d0, d1 = abs(float(s0) - ref.sum()), abs(float(s1) - (c * ref).sum())
        print(f"{W}x{H} {np.dtype(dt).name} r={r} f={p} guides {mask}: |sum - ref| {d0:.3e} (bound {tol.sum():.3e}), "
              f"weighted {d1:.3e} (bound {(c * tol).sum():.3e})")
        assert d0 <= tol.sum() and d1 <= (c * tol).sum()
