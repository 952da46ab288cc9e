#!/usr/bin/env python3
"""Sigma sweep of rt_denoise_guided on one config: the RMSE (after the output's gamma, against a
uniform render at 4 x spp under another seed, as scripts/adaptive_bench.py) of the adaptive frame
unfiltered, through rt_denoise, and through rt_denoise_guided with rt_render_features' buffers at
16 spp for every sigma triple of {0.05, 0.1, 0.2, 0.4}^3 and for each guide alone, at the filter
parameters (10, 3, 0.45) and (5, 2, 1.0).

usage: python scripts/guided_sweep.py C2|C3 THRESHOLD [OUT.json]
"""
import itertools, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import __graft_entry__ as ge
rt = ge.import_binding()
CONFIGS = {"C2": dict(scene=0, width=1200, height=800, spp=500), "C3": dict(scene=5, width=800, height=800, spp=1000)}
name, thr = sys.argv[1], float(sys.argv[2])
c = CONFIGS[name]
W, H, spp = c["width"], c["height"], c["spp"]
r = rt.Renderer(0)
r.upload(rt.World(1).build_scene(c["scene"]))
cam, bg = rt.scene_camera(c["scene"], W, H)
gamma = lambda x: np.sqrt(np.clip(x.astype(np.float64), 0.0, 0.999))
rmse = lambda x: float(np.sqrt(np.mean((gamma(x) - ref) ** 2)))
ref = gamma(r.render(cam, rt.Renderer.params(W, H, spp * 4, 50, bg, 2, out_format=rt.RT_OUT_F32)))
p = rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=rt.RT_OUT_F32)
img, tile_spp, _, se = r.render_adaptive(cam, p, 64, 64, thr)
a, n, z = r.render_features(cam, rt.Renderer.params(W, H, 16, 50, bg, 1, out_format=rt.RT_OUT_F64))
out = dict(config=name, threshold=thr, build=rt.build_info(), mean_tile_spp=float(tile_spp.mean()), features_spp=16, results=[])
for R, F, K in ((10, 3, 0.45), (5, 2, 1.0)):
    e = dict(params=[R, F, K], rmse=rmse(img), rmse_plain=rmse(r.denoise(img, se, R, F, K)), triples=[], singles=[])
    grid = (0.05, 0.1, 0.2, 0.4)
    for sa, sn, sz in itertools.product(grid, grid, grid):
        e["triples"].append([sa, sn, sz, rmse(r.denoise_guided(img, se, a, n, z, (sa, sn, sz), R, F, K))])
    for i, s in itertools.product(range(3), grid):
        g = [a, n, z]
        g = [x if j == i else None for j, x in enumerate(g)]
        e["singles"].append([i, s, rmse(r.denoise_guided(img, se, *g, (s, s, s), R, F, K))])
    e["best"] = min(e["triples"], key=lambda t: t[3])
    print(name, thr, (R, F, K), "rmse", e["rmse"], "plain", e["rmse_plain"], "best", e["best"], flush=True)
    out["results"].append(e)
json.dump(out, open(sys.argv[3] if len(sys.argv) > 3 else f"guided_sweep_{name.lower()}.json", "w"), indent=1)
