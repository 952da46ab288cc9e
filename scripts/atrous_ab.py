#!/usr/bin/env python3
"""A/B of rt_denoise_atrous's level kernels between builds of the library (the direct gather
against the LDS-staged tile at step 1, or at steps 1 and 2: -DRT_ATROUS_LDS_STEPS=1 / 2 builds made
with __graft_entry__.build_library(extra_flags=[...], name=...)).

One child process per library (RT_LIB_PATH picks the .so), the children one after another, ROUNDS
times round-robin. A child renders the config's adaptive frame at threshold 0.02 (f32) and its
16-spp guides once, then times the filter (kernel ms, HIP events) at L = 1, 2, 3 and 5, guided and
demodulated, guided, and unguided, 3 calls each per round after one warm-up; it also prints a
checksum of every output so the builds' bits can be compared. L = 1 is the step-1 level alone (a
first-and-last launch), L = 2 minus L = 1 about the step-2 level, and so on.

usage: python scripts/atrous_ab.py C2|C3 NAME=LIB.so [NAME=LIB.so ...]
"""
import json, os, subprocess, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = 3
CONFIGS = {"C2": dict(scene=0, width=1200, height=800, spp=500), "C3": dict(scene=5, width=800, height=800, spp=1000)}

CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, {repo!r})
import numpy as np
import __graft_entry__ as ge
rt = ge.import_binding()
c = json.loads({cfg!r})
W, H, spp = c["width"], c["height"], c["spp"]
r = rt.Renderer(0)
r.upload(rt.World(1).build_scene(c["scene"]))
cam, bg = rt.scene_camera(c["scene"], W, H)
img, _, _, se = r.render_adaptive(cam, rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=rt.RT_OUT_F32), 64, 64, 0.02)
a, n, z = r.render_features(cam, rt.Renderer.params(W, H, 16, 50, bg, 1, out_format=rt.RT_OUT_F64))
res = {{}}
for L in (1, 2, 3, 5):
    for what, g, dem in (("demodulated", (a, n, z), True), ("guided", (a, n, z), False), ("unguided", (None, None, None), False)):
        call = lambda: r.denoise_atrous(img, se, *g, rt.GUIDE_SIGMAS, L, 4.0, dem)
        out, so = call()
        ms = []
        for _ in range(3):
            call()
            ms.append(r.atrous_stats().kernel_ms)
        res[f"L{{L}} {{what}}"] = dict(ms=ms, sha=hashlib.sha256(out.tobytes() + so.tobytes()).hexdigest()[:12])
print("RESULT", json.dumps(res))
print("BUILD", rt.build_info())
"""


def main():
    cfg = CONFIGS[sys.argv[1]]
    libs = [x.split("=", 1) for x in sys.argv[2:]]
    runs, shas = {}, {}
    for _ in range(ROUNDS):
        for name, lib in libs:
            env = dict(os.environ, RT_LIB_PATH=os.path.abspath(lib))
            out = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, cfg=json.dumps(cfg))], env=env,
                                 capture_output=True, text=True, timeout=240)
            if out.returncode != 0:
                print(f"{name}: child failed ({out.returncode})\n{out.stderr[-2000:]}")
                sys.exit(out.returncode if out.returncode > 0 else 1)
            d = json.loads([x for x in out.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
            build = [x for x in out.stdout.splitlines() if x.startswith("BUILD ")][-1][6:]
            for k, e in d.items():
                runs.setdefault((name, build, k), []).extend(e["ms"])
                shas.setdefault(k, {})[name] = e["sha"]
    for (name, build, k), ms in runs.items():
        ms.sort()
        print(f"{sys.argv[1]} {name} build {build} {k}: kernel ms median {ms[len(ms) // 2]:.4f} ({ms[0]:.4f}-{ms[-1]:.4f}) of {len(ms)}, "
              f"sha {shas[k][name]}", flush=True)
    for k, by in shas.items():
        print(f"{sys.argv[1]} {k}: outputs {'equal' if len(set(by.values())) == 1 else 'DIFFER'} across builds")


if __name__ == "__main__":
    main()
