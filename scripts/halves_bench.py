#!/usr/bin/env python3
"""What rt_render_adaptive_halves costs over rt_render_adaptive, and whether rt_render_adaptive
itself moved against another build.

Each library runs in its own child process (RT_LIB_PATH picks the .so), the children one after
another, `--rounds` times round-robin; inside a child the modes (plain / halves at each threshold)
alternate `--reps` times after one warm-up each, so clock drift spreads over everything compared. A
library without rt_render_adaptive_halves (a build of the commit before, given with --parent) runs
the plain mode only, and then so does a third child of this build ("new-alone"): the like-for-like
comparison of the plain call across builds. Reported per (library, mode, threshold): the median and min-max of the
synchronous host-pointer call's wall ms (f32 frame) and of the moments kernels' HIP-event ms
(rt_adaptive_stats.moments_ms), with the trace ms beside them.

usage: python scripts/halves_bench.py --config C2 --thresholds 0 0.02 [--parent lib/librtiow_parent.so]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {   # bench.py's
    "C2": dict(scene=0, width=1200, height=800, spp=500, depth=50),
    "C3": dict(scene=5, width=800, height=800, spp=1000, depth=50),
    "C4": dict(scene=7, width=1920, height=1080, spp=1000, depth=50),
}

CHILD = r"""
import json, sys, time
sys.path.insert(0, {repo!r})
import __graft_entry__ as ge
rt = ge.import_binding()
a = json.loads({args!r})
W, H, spp = a["width"], a["height"], a["spp"]
cam, bg = rt.scene_camera(a["scene"], W, H)
r = rt.Renderer(0)
r.upload(rt.World(1).build_scene(a["scene"]))
has_halves = hasattr(r.lib, "rt_render_adaptive_halves") and not a["plain_only"]
modes = [(m, t) for t in a["thresholds"] for m in (("plain", "halves") if has_halves else ("plain",))]
def run(mode, t):
    p = rt.Renderer.params(W, H, spp, a["depth"], bg, 1, out_format=rt.RT_OUT_F32)
    call = r.render_adaptive_halves if mode == "halves" else r.render_adaptive
    t0 = time.perf_counter()
    call(cam, p, a["min_spp"], a["step_spp"], t)
    ms = (time.perf_counter() - t0) * 1e3
    st = r.adaptive_stats()
    return dict(wall_ms=ms, moments_ms=st.moments_ms, trace_ms=st.trace_ms, passes=st.passes, samples=st.samples_traced)
res = dict()
for m, t in modes:
    run(m, t)
for _ in range(a["reps"]):
    for m, t in modes:
        res.setdefault(m + ":" + repr(t), []).append(run(m, t))
print("RESULT", json.dumps(res))
print("BUILD", rt.build_info())
"""


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=sorted(CONFIGS))
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.0, 0.02])
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--step-spp", type=int, default=64)
    ap.add_argument("--parent", default=None, help="a library built from the commit before (plain mode only)")
    ap.add_argument("--lib", default=os.path.join("rust-ray-tracing-in-a-weekend_amd", "lib", "librtiow_amd.so"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    # with a parent: this build once more with the plain mode alone, as the parent's child runs it (a
    # plain call after a halves call finds the allocator in another state than one after a plain call)
    jobs = [("new", a.lib)] + ([("new-alone", a.lib), ("parent", a.parent)] if a.parent else [])
    runs, builds = {}, {}
    for _ in range(a.rounds):
        for name, lib in jobs:
            args = dict(CONFIGS[a.config], thresholds=a.thresholds, reps=a.reps, min_spp=a.min_spp, step_spp=a.step_spp,
                        plain_only=name == "new-alone")
            env = dict(os.environ, RT_LIB_PATH=os.path.abspath(os.path.join(REPO, lib)))
            out = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, args=json.dumps(args))], env=env,
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                print(f"{name}: child failed ({out.returncode})\n{out.stderr[-2000:]}")
                sys.exit(out.returncode if out.returncode > 0 else 1)
            d = json.loads([x for x in out.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
            builds[name] = [x for x in out.stdout.splitlines() if x.startswith("BUILD ")][-1][6:]
            for mode, rs in d.items():
                runs.setdefault(f"{name}:{mode}", []).extend(rs)
    for name, b in builds.items():
        print(f"{a.config} {name}: rt_build_info {b}")
    for key, rs in runs.items():
        s = dict(n=len(rs), passes=rs[0]["passes"], samples=rs[0]["samples"])
        for f in ("wall_ms", "moments_ms", "trace_ms"):
            v = [x[f] for x in rs]
            s[f] = [round(med(v), 4), round(min(v), 4), round(max(v), 4)]   # median, min, max
        print(f"{a.config} {key}: " + json.dumps(s))


if __name__ == "__main__":
    main()
