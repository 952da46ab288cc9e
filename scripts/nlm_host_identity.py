#!/usr/bin/env python3
"""The host NL-means filters (rt_denoise_host, rt_denoise_guided_host, rt_denoise_cross_host,
rt_denoise_pyramid_host) of two builds of the library compared bit for bit. A parent build is made
with __graft_entry__.build_library(csrc=<the parent commit's csrc>, name="librtiow_parent.so").
Every library runs in a child process of its own (RT_LIB_PATH). No GPU.

    python scripts/nlm_host_identity.py PARENT.so NEW.so

The frames are the CPU tests' (tests/denoise_reference.py CPU_INPUTS and the pyramid's odd sizes,
cast to f32 and to f64) at those tests' parameter sets, unguided and guided, cross with and without
stderr_out: one sha256 per output and library. Exit status 1 if any output differs. A one-off check
of a change to the host filters, not a test: libm's exp is not fixed across machines.
"""
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sha(*arrays) -> str:
    return hashlib.sha256(b"".join(a.tobytes() for a in arrays if a is not None)).hexdigest()[:16]


def child():
    import numpy as np
    sys.path.insert(0, REPO)
    import __graft_entry__ as ge
    from tests import denoise_cross_reference as cr, denoise_guided_reference as gr, denoise_pyramid_reference as pr
    from tests import denoise_reference as dr
    rt = ge.import_binding()
    res = {}
    for name in dr.CPU_INPUTS:
        mean, se = dr.cpu_input(name)
        a, b, _ = cr.cpu_input(name)
        guides = gr.cpu_guides(mean)
        for dt in (np.float32, np.float64):
            m, ha, hb = (x.astype(dt) for x in (mean, a, b))
            for r, f, k in dr.PARAMS:
                key = f"{name} {np.dtype(dt).name} ({r}, {f}, {k})"
                res[key + " denoise"] = sha(rt.denoise_host(m, se, r, f, k))
                res[key + " guided"] = sha(rt.denoise_guided_host(m, se, *guides, gr.SIGMAS, r, f, k))
                for g, gk in (("", {}), (" guided", dict(zip(("albedo", "normal", "depth"), guides), sigmas=gr.SIGMAS))):
                    for want in (True, False):
                        out = rt.denoise_cross_host(ha, hb, se, radius=r, patch=f, k=k, variance_scale=cr.SCALE,
                                                    want_stderr=want, **gk)
                        res[f"{key} cross{g}{'' if want else ' no stderr_out'}"] = sha(*out)
    for name in pr.CPU_FRAMES:
        mean, se = pr.cpu_frame(name)
        for dt in (np.float32, np.float64):
            for r, f, k in pr.PARAMS:
                for guided in (False, True):
                    out = rt.denoise_pyramid_host(mean.astype(dt), se, *pr.guides_for(mean, guided), pr.SIGMAS, r, f, k, 3)
                    res[f"{name} {np.dtype(dt).name} ({r}, {f}, {k}) pyramid{' guided' if guided else ''}"] = sha(out)
    print("RESULT", json.dumps(res))
    print("BUILD", rt.build_info())


def run_child(lib):
    env = dict(os.environ, RT_LIB_PATH=os.path.abspath(lib))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=env, capture_output=True, text=True,
                         timeout=900)
    if out.returncode != 0:
        print(f"{lib}: child failed ({out.returncode})\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}", flush=True)
        sys.exit(out.returncode if out.returncode > 0 else 1)
    lines = out.stdout.splitlines()
    return (json.loads([x for x in lines if x.startswith("RESULT ")][-1][7:]),
            [x for x in lines if x.startswith("BUILD ")][-1][6:])


def main():
    if sys.argv[1] == "child":
        return child()
    (pa, pb), (na, nb) = run_child(sys.argv[1]), run_child(sys.argv[2])
    print(f"parent build {pb}, new build {nb}")
    differ = 0
    for k in pa:
        differ += pa[k] != na[k]
        print(f"{k}: parent {pa[k]} new {na[k]} {'equal' if pa[k] == na[k] else 'DIFFER'}")
    print(f"{len(pa)} outputs, {differ} differ")
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
