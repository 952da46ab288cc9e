"""rt_denoise_pyramid_host under ASan and UBSan, built the way tests/test_denoise_atrous_sanitized.py
builds its program.

tests/pyramid_host_main.cpp has its own main and links csrc/pyramid_host.cpp and
csrc/denoise_host.cpp alone (no HIP include path, no HIP library). The program itself is
instrumented and run directly: nothing is preloaded. Every buffer — the frame, the map, the guides,
the output — is exactly its frame's size, so a read or write past an edge is reported. It prints two
checksums per case (sum_i x_i and sum_i c_i x_i, c_i = 1 + i mod 7); the same sums of the numpy
reference (tests/denoise_pyramid_reference.py) must agree within sum_i c_i (1e-11 + 1e-11 |ref_i|),
the per-element tolerance summed. The sizes are the odd ones of the host test: levels of one pixel,
blocks of one and two pixels, clamped taps on both axes.
"""
import os
import re
import struct
import subprocess

import numpy as np

from tests import denoise_atrous_reference as atr
from tests import denoise_pyramid_reference as pr
from tests import denoise_reference as dr
from tests.test_denoise_sanitized import CLANG, CSRC, FLAGS, REPO

SOURCES = [os.path.join(REPO, "tests", "pyramid_host_main.cpp"), os.path.join(CSRC, "pyramid_host.cpp"),
           os.path.join(CSRC, "denoise_host.cpp")]

#        W,  H, dtype,      radius, patch, k, levels, guide mask (1 albedo, 2 normal, 4 depth)
CASES = [(1, 1, np.float64, 3, 1, 0.45, 5, 0),
         (1, 1, np.float32, 5, 2, 1.0, 2, 7),
         (2, 1, np.float64, 5, 2, 1.0, 3, 7),
         (2, 1, np.float32, 3, 1, 0.45, 5, 0),
         (3, 3, np.float64, 3, 1, 0.45, 2, 5),
         (3, 3, np.float32, 5, 2, 1.0, 5, 7),
         (9, 5, np.float64, 5, 2, 1.0, 5, 7),
         (9, 5, np.float32, 3, 1, 0.45, 3, 2),
         (72, 9, np.float64, 3, 1, 0.45, 5, 0),
         (72, 9, np.float32, 5, 2, 1.0, 4, 7),
         (9, 5, np.float32, 10, 3, 0.45, 1, 7)]    # one level: the filter itself on the caller's buffers


def test_pyramid_host_filter_is_clean_under_asan_and_ubsan(tmp_path):
    exe, data = str(tmp_path / "pyramid_host_main"), str(tmp_path / "cases.bin")
    b = subprocess.run([CLANG, *FLAGS, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    frames = [pr.odd_frame(W, H, dt, i) for i, (W, H, dt, *_rest) in enumerate(CASES)]
    guides = []
    with open(data, "wb") as f:
        f.write(struct.pack("<i", len(CASES)))
        for (W, H, dt, r, p, k, levels, mask), (mean, se) in zip(CASES, frames):
            g = [x if mask >> i & 1 else None for i, x in enumerate(atr.coord_guides(H, W))]
            guides.append(g)
            f.write(struct.pack("<7i4d", W, H, 1 if dt == np.float64 else 0, r, p, levels, mask, k, *pr.SIGMAS))
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
    for (W, H, dt, r, p, k, levels, mask), (mean, se), g, (_, s0, s1) in zip(CASES, frames, guides, sums):
        ref = pr.pyramid(mean, se, r, p, k, levels, *g, pr.SIGMAS).astype(np.float64).reshape(-1)
        c = 1.0 + np.arange(ref.size) % 7
        if dt == np.float32:     # one f32 ulp of each rounded reference value
            tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        else:
            tol = dr.TOL_ABS + dr.TOL_REL * np.abs(ref)
        d0, d1 = abs(float(s0) - ref.sum()), abs(float(s1) - (c * ref).sum())
        print(f"{W}x{H} {np.dtype(dt).name} r={r} f={p} L={levels} guides {mask}: |sum - ref| {d0:.3e} "
              f"(bound {tol.sum():.3e}), weighted {d1:.3e} (bound {(c * tol).sum():.3e})")
        assert d0 <= tol.sum() and d1 <= (c * tol).sum()
