#!/usr/bin/env python3
"""What an rt_adaptive_state costs beside rt_render_adaptive, and what refining a frame saves over
rendering it again.

One child process per library (RT_LIB_PATH picks the .so), the children one after another,
`--rounds` times round-robin. Inside the child of this build the alternatives alternate `--reps`
times after one warm-up each, so clock drift spreads over everything compared:
  one:T      rt_render_adaptive at threshold T (host pointers, f32 frame)
  fresh:T    a fresh state advanced to T and resolved (create and destroy inside the timing)
  refine     a state at --threshold advanced to --refine and resolved (the second stage alone)
A library without the state symbols (a build of the commit before, given with --parent) runs
one:T only. Reported per (library, mode): median, min and max of the wall ms, of the trace, moments
and classify HIP-event ms, the groups (or passes), classify ms per launch, and once per child the
tiles of every group of the refining stage. Every line carries the library's rt_build_info.

usage: python scripts/adaptive_state_bench.py --config C2 [--parent lib/librtiow_parent.so]
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
W, H, spp, T1, T2 = a["width"], a["height"], a["spp"], a["threshold"], a["refine"]
cam, bg = rt.scene_camera(a["scene"], W, H)
r = rt.Renderer(0)
r.upload(rt.World(1).build_scene(a["scene"]))
has_state = hasattr(r.lib, "rt_adaptive_state_create")
def params():
    return rt.Renderer.params(W, H, spp, a["depth"], bg, 1, out_format=rt.RT_OUT_F32)
def one(t):
    t0 = time.perf_counter()
    r.render_adaptive(cam, params(), a["min_spp"], a["step_spp"], t)
    ms = (time.perf_counter() - t0) * 1e3
    st = r.adaptive_stats()
    return dict(wall_ms=ms, trace_ms=st.trace_ms, moments_ms=st.moments_ms, classify_ms=st.classify_ms,
                launches=st.passes, classify_launches=st.passes, samples=st.samples_traced)
def state_stats(ms, s, fresh):
    return dict(wall_ms=ms, trace_ms=s.trace_ms, moments_ms=s.moments_ms, classify_ms=s.classify_ms, launches=s.groups,
                classify_launches=s.groups + (0 if fresh else 1), samples=s.samples_traced)
def fresh(t):
    t0 = time.perf_counter()
    st = r.adaptive_state(cam, params(), a["min_spp"], a["step_spp"])
    st.advance(t, spp)
    st.resolve(rt.RT_OUT_F32)
    s = st.stats()
    st.close()
    return state_stats((time.perf_counter() - t0) * 1e3, s, True)
def refine(split=False):
    st = r.adaptive_state(cam, params(), a["min_spp"], a["step_spp"])
    st.advance(T1, spp)
    st.resolve(rt.RT_OUT_F32)
    if split:   # (untimed) the tiles of every group of the second stage
        tiles, prev = [], st.resolve(rt.RT_OUT_F32)[1]
        while True:
            st.advance(T2, spp, max_launches=1)
            if not st.stats().groups:
                break
            cur = st.resolve(rt.RT_OUT_F32)[1]
            tiles.append(int((cur != prev).sum()))
            prev = cur
        st.close()
        return tiles
    t0 = time.perf_counter()
    st.advance(T2, spp)
    st.resolve(rt.RT_OUT_F32)
    ms = (time.perf_counter() - t0) * 1e3
    s = st.stats()
    st.close()
    return state_stats(ms, s, False)
modes = [("one:" + repr(T1), lambda: one(T1))]
if has_state and not a["plain_only"]:
    modes += [("fresh:" + repr(T1), lambda: fresh(T1)), ("one:" + repr(T2), lambda: one(T2)),
              ("fresh:" + repr(T2), lambda: fresh(T2)), ("refine", refine)]
res = dict()
for _, f in modes:
    f()
for _ in range(a["reps"]):
    for m, f in modes:
        res.setdefault(m, []).append(f())
if has_state and not a["plain_only"]:
    s = r.adaptive_state(cam, params(), a["min_spp"], a["step_spp"]).stats()
    print("GROUPS", json.dumps(dict(step_r=s.step_spp, min_r=s.min_spp, chunk=s.spp_chunk, tiles=s.tiles,
                                    refine_group_tiles=refine(split=True))))
print("RESULT", json.dumps(res))
print("BUILD", rt.build_info())
"""


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=sorted(CONFIGS))
    ap.add_argument("--threshold", type=float, default=0.02)
    ap.add_argument("--refine", type=float, default=0.01)
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--step-spp", type=int, default=64)
    ap.add_argument("--parent", default=None, help="a library built from the commit before (one:T only)")
    ap.add_argument("--lib", default=os.path.join("rust-ray-tracing-in-a-weekend_amd", "lib", "librtiow_amd.so"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    jobs = [("new", a.lib)] + ([("new-alone", a.lib), ("parent", a.parent)] if a.parent else [])
    runs, builds, groups = {}, {}, None
    for _ in range(a.rounds):
        for name, lib in jobs:
            args = dict(CONFIGS[a.config], threshold=a.threshold, refine=a.refine, reps=a.reps, min_spp=a.min_spp,
                        step_spp=a.step_spp, plain_only=name == "new-alone")
            env = dict(os.environ, RT_LIB_PATH=os.path.abspath(os.path.join(REPO, lib)))
            out = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, args=json.dumps(args))], env=env,
                                 capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                print(f"{name}: child failed ({out.returncode})\n{out.stderr[-2000:]}")
                sys.exit(out.returncode if out.returncode > 0 else 1)
            lines = out.stdout.splitlines()
            d = json.loads([x for x in lines if x.startswith("RESULT ")][-1][7:])
            builds[name] = [x for x in lines if x.startswith("BUILD ")][-1][6:]
            g = [x for x in lines if x.startswith("GROUPS ")]
            if g:
                groups = (name, json.loads(g[-1][7:]))
            for mode, rs in d.items():
                runs.setdefault((name, mode), []).extend(rs)
    if groups:
        print(f"{a.config} {groups[0]} [{builds[groups[0]]}] groups: " + json.dumps(groups[1]))
    for (name, mode), rs in runs.items():
        s = dict(n=len(rs), launches=rs[0]["launches"], samples=rs[0]["samples"])
        for f in ("wall_ms", "trace_ms", "moments_ms", "classify_ms"):
            v = [x[f] for x in rs]
            s[f] = [round(med(v), 4), round(min(v), 4), round(max(v), 4)]   # median, min, max
        s["classify_ms_per_launch"] = round(med([x["classify_ms"] / max(x["classify_launches"], 1) for x in rs]), 4)
        print(f"{a.config} {name}:{mode} [{builds[name]}]: " + json.dumps(s))


if __name__ == "__main__":
    main()
