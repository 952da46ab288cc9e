#!/usr/bin/env python3
"""Sweep of rt_denoise_pyramid on one config, beside rt_denoise on the same frame in the same
process: the adaptive frame at THRESHOLD (f32, scripts/adaptive_bench.py's settings), windows
(5, 2, 1.0) and (10, 3, 0.45), levels {1, 2, 3, 4}, unguided; on C2 also guided by
rt_render_features' buffers at 16 spp with the binding's sigmas.

Per line: the RMSE (after the output's gamma, against a uniform render at 4 x spp under another
seed) and the kernels' HIP-event time as the median of REPS calls with min and max,
each call followed by one rt_denoise (guided lines: rt_denoise_guided) call with the same window,
whose median is the line's yardstick: ratio = pyramid / plain.

usage: python scripts/pyramid_sweep.py C2|C3|C4 THRESHOLD [OUT.json]
"""
import json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import __graft_entry__ as ge
rt = ge.import_binding()
CONFIGS = {"C2": dict(scene=0, width=1200, height=800, spp=500), "C3": dict(scene=5, width=800, height=800, spp=1000),
           "C4": dict(scene=7, width=1920, height=1080, spp=1000)}
REPS = 7
WINDOWS = ((5, 2, 1.0), (10, 3, 0.45))
LEVELS = (1, 2, 3, 4)
name, thr = sys.argv[1], float(sys.argv[2])
c = CONFIGS[name]
W, H, spp = c["width"], c["height"], c["spp"]
r = rt.Renderer(0)
r.upload(rt.World(1).build_scene(c["scene"]))
cam, bg = rt.scene_camera(c["scene"], W, H)
gamma = lambda x: np.sqrt(np.clip(x.astype(np.float64), 0.0, 0.999))
ref = gamma(r.render(cam, rt.Renderer.params(W, H, spp * 4, 50, bg, 2, out_format=rt.RT_OUT_F32)))
rmse = lambda x: float(np.sqrt(np.mean((gamma(x) - ref) ** 2)))
p = rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=rt.RT_OUT_F32)
img, tile_spp, _, se = r.render_adaptive(cam, p, 64, 64, thr)
guides = r.render_features(cam, rt.Renderer.params(W, H, 16, 50, bg, 1, out_format=rt.RT_OUT_F64)) if name == "C2" else None
build = rt.build_info()


def med(ms):
    ms = sorted(ms)
    return [ms[len(ms) // 2], ms[0], ms[-1]]


def timed(pyramid, plain):
    """(the pyramid's result, its [median, min, max] kernel ms, the plain filter's) of REPS interleaved
    pairs of calls after one warm-up pair."""
    pyramid(), plain()
    a, b = [], []
    for _ in range(REPS):
        res = pyramid()
        a.append(r.pyramid_stats().kernel_ms)
        plain()
        b.append(r.denoise_stats().kernel_ms)
    return res, med(a), med(b)


out = dict(config=name, threshold=thr, build=build, mean_tile_spp=float(tile_spp.mean()), rmse=rmse(img),
           mean_se=float(se.mean()), reps=REPS, lines=[])
print(f"{name} {thr} build {build}: unfiltered rmse {out['rmse']:.6f}, mean se {out['mean_se']:.6f}, "
      f"mean tile spp {out['mean_tile_spp']:.1f}", flush=True)
for g, label in ((None, "unguided"), (guides, "guided")):
    if label == "guided" and g is None:
        continue
    ga = g if g is not None else (None, None, None)
    for R, F, K in WINDOWS:
        for L in LEVELS:
            f, ms, ms_plain = timed(lambda: r.denoise_pyramid(img, se, *ga, rt.GUIDE_SIGMAS, R, F, K, L),
                                    lambda: r.denoise_guided(img, se, *ga, rt.GUIDE_SIGMAS, R, F, K))
            e = dict(guides=label, params=[R, F, K], levels=L, rmse=rmse(f), kernel_ms=ms, plain_ms=ms_plain,
                     ratio=ms[0] / ms_plain[0], scratch_bytes=int(r.pyramid_stats().scratch_bytes))
            out["lines"].append(e)
            print(f"{name} build {build} pyramid {label} {(R, F, K)} L={L}: rmse {e['rmse']:.6f} ms {ms[0]:.3f} "
                  f"({ms[1]:.3f}-{ms[2]:.3f}); one level beside it {ms_plain[0]:.3f} ({ms_plain[1]:.3f}-{ms_plain[2]:.3f}); "
                  f"ratio {e['ratio']:.3f}; scratch {e['scratch_bytes']} B", flush=True)
json.dump(out, open(sys.argv[3] if len(sys.argv) > 3 else f"pyramid_sweep_{name.lower()}.json", "w"), indent=1)
