#!/usr/bin/env python3
"""Sweep of rt_denoise_atrous on one config, beside rt_denoise and rt_denoise_guided on the same
frame in the same process: the adaptive frame at THRESHOLD (f32, scripts/adaptive_bench.py's
settings), rt_render_features' buffers at 16 spp with the binding's sigmas, levels {3, 4, 5} x
sigma_l {1, 2, 4, 8} x demodulate {off, on}; NL-means at (10, 3, 0.45) and (5, 2, 1.0), plain and
guided.

Per filter: the RMSE (after the output's gamma, against a uniform render at 4 x spp under another
seed) and the kernel's HIP-event time as the median of 9 calls with min and max. Per
a-trous line also: the mean of stderr_out beside the RMSE the filtered frame's luminance really has
against the reference (linear space, what stderr_out estimates), and the fraction of the memory
floor (64 B per pixel and level at 5.95 TB/s) the kernels reach.

usage: python scripts/atrous_sweep.py C2|C3|C4 THRESHOLD [OUT.json]
"""
import itertools, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import __graft_entry__ as ge
rt = ge.import_binding()
CONFIGS = {"C2": dict(scene=0, width=1200, height=800, spp=500), "C3": dict(scene=5, width=800, height=800, spp=1000),
           "C4": dict(scene=7, width=1920, height=1080, spp=1000)}
REPS = 9
FLOOR_BPS = 5.95e12
name, thr = sys.argv[1], float(sys.argv[2])
c = CONFIGS[name]
W, H, spp = c["width"], c["height"], c["spp"]
r = rt.Renderer(0)
r.upload(rt.World(1).build_scene(c["scene"]))
cam, bg = rt.scene_camera(c["scene"], W, H)
gamma = lambda x: np.sqrt(np.clip(x.astype(np.float64), 0.0, 0.999))
luma = lambda x: 0.2126 * x[..., 0].astype(np.float64) + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]
ref_lin = r.render(cam, rt.Renderer.params(W, H, spp * 4, 50, bg, 2, out_format=rt.RT_OUT_F32))
ref = gamma(ref_lin)
rmse = lambda x: float(np.sqrt(np.mean((gamma(x) - ref) ** 2)))
rmse_luma = lambda x: float(np.sqrt(np.mean((luma(x) - luma(ref_lin)) ** 2)))
p = rt.Renderer.params(W, H, spp, 50, bg, 1, out_format=rt.RT_OUT_F32)
img, tile_spp, _, se = r.render_adaptive(cam, p, 64, 64, thr)
a, n, z = r.render_features(cam, rt.Renderer.params(W, H, 16, 50, bg, 1, out_format=rt.RT_OUT_F64))
build = rt.build_info()


def timed(call, stats):
    """(the last result, [median, min, max] kernel ms) of REPS calls after one warm-up."""
    call()
    ms = []
    for _ in range(REPS):
        res = call()
        ms.append(stats().kernel_ms)
    ms.sort()
    return res, [ms[len(ms) // 2], ms[0], ms[-1]]


out = dict(config=name, threshold=thr, build=build, mean_tile_spp=float(tile_spp.mean()), features_spp=16,
           guide_sigmas=list(rt.GUIDE_SIGMAS), rmse=rmse(img), rmse_luma_linear=rmse_luma(img), mean_se=float(se.mean()),
           nlm=[], atrous=[])
print(f"{name} {thr} build {build}: unfiltered rmse {out['rmse']:.6f}, luminance rmse (linear) {out['rmse_luma_linear']:.6f}, "
      f"mean se {out['mean_se']:.6f}, mean tile spp {out['mean_tile_spp']:.1f}", flush=True)
for R, F, K in ((10, 3, 0.45), (5, 2, 1.0)):
    plain, ms_p = timed(lambda: r.denoise(img, se, R, F, K), r.denoise_stats)
    guided, ms_g = timed(lambda: r.denoise_guided(img, se, a, n, z, rt.GUIDE_SIGMAS, R, F, K), r.denoise_stats)
    e = dict(params=[R, F, K], rmse_plain=rmse(plain), plain_ms=ms_p, rmse_guided=rmse(guided), guided_ms=ms_g)
    out["nlm"].append(e)
    print(f"{name} build {build} nlm {(R, F, K)}: plain rmse {e['rmse_plain']:.6f} ms {ms_p[0]:.3f} ({ms_p[1]:.3f}-{ms_p[2]:.3f}); "
          f"guided rmse {e['rmse_guided']:.6f} ms {ms_g[0]:.3f} ({ms_g[1]:.3f}-{ms_g[2]:.3f})", flush=True)
for dem, L, sl in itertools.product((False, True), (3, 4, 5), (1.0, 2.0, 4.0, 8.0)):
    (f, f_se), ms = timed(lambda: r.denoise_atrous(img, se, a, n, z, rt.GUIDE_SIGMAS, L, sl, dem), r.atrous_stats)
    floor_ms = 64.0 * W * H * L / FLOOR_BPS * 1e3
    e = dict(levels=L, sigma_l=sl, demodulate=int(dem), rmse=rmse(f), kernel_ms=ms, rmse_luma_linear=rmse_luma(f),
             mean_stderr_out=float(f_se.mean()), floor_ms=floor_ms, floor_fraction=floor_ms / ms[0],
             scratch_bytes=int(r.atrous_stats().scratch_bytes))
    out["atrous"].append(e)
    print(f"{name} build {build} atrous L={L} sigma_l={sl:g} demodulate={int(dem)}: rmse {e['rmse']:.6f} ms {ms[0]:.3f} "
          f"({ms[1]:.3f}-{ms[2]:.3f}) floor {floor_ms:.4f} ms = {e['floor_fraction']:.3f} of the time; luminance rmse "
          f"(linear) {e['rmse_luma_linear']:.6f}, mean stderr_out {e['mean_stderr_out']:.6f}", flush=True)
# without guides, at the best guided setting of each demodulate = 0 level count
for L in (3, 4, 5):
    best = min((e for e in out["atrous"] if e["levels"] == L and not e["demodulate"]), key=lambda e: e["rmse"])
    (f, f_se), ms = timed(lambda: r.denoise_atrous(img, se, None, None, None, rt.GUIDE_SIGMAS, L, best["sigma_l"]), r.atrous_stats)
    e = dict(levels=L, sigma_l=best["sigma_l"], rmse=rmse(f), kernel_ms=ms, mean_stderr_out=float(f_se.mean()))
    out.setdefault("atrous_unguided", []).append(e)
    print(f"{name} build {build} atrous unguided L={L} sigma_l={best['sigma_l']:g}: rmse {e['rmse']:.6f} ms {ms[0]:.3f} "
          f"({ms[1]:.3f}-{ms[2]:.3f})", flush=True)
out["best"] = min(out["atrous"], key=lambda e: e["rmse"])
print(f"{name} build {build} best", json.dumps(out["best"]), flush=True)
json.dump(out, open(sys.argv[3] if len(sys.argv) > 3 else f"atrous_sweep_{name.lower()}.json", "w"), indent=1)
