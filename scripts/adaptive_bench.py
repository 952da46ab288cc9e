#!/usr/bin/env python3
"""Tile-adaptive sampling (rt_render_adaptive) against the uniform rt_render on one config:
overhead (threshold 0: the same samples in passes, through the moments kernel) and gain
(samples traced, wall time and image error at a few thresholds).

Each (library, mode list) runs in its own child process (RT_LIB_PATH picks the .so), the children
one after another, `--rounds` times round-robin, and inside a child the modes alternate, so clock
drift spreads over everything compared. A parent build (lib/librtiow_parent.so, built with
__graft_entry__.build_library(csrc=<the parent commit's csrc>, name="librtiow_parent.so")) given
with --parent runs the uniform mode only: it has no adaptive call.

Times: wall ms of the synchronous call with a host f32 frame (host clock around a call that ends
in a stream synchronise), and the HIP-event times the library reports. Bytes/s of the reductions:
the per-sample records they read (24 B x samples traced) over their event time.
Error: RMSE of sqrt(clamp(mean, 0, 0.999)) (the output's gamma) against a uniform render at
--ref-mult x spp under another render seed, so the reference shares no sample with either frame.
--denoise R F K: every mode's frame also goes through rt_denoise (radius R, patch F, k K) with the
error map of its own adaptive call (the uniform frame: of an adaptive call at threshold 0, which
renders the same frame); reported are rmse_denoised beside rmse, the filter kernel's HIP-event time
and the wall time of the host-pointer call (copies included). Without it the output is unchanged.
--features SPP: every repetition also times the first-hit feature pass (rt_render_features at SPP
samples per pixel): its HIP-event time (trace_features + its reduction) and the host-pointer call's
wall time. --guided SA SN SZ (with --denoise): after the plain filter the same frame goes through
rt_denoise_guided with the feature buffers (at --features SPP, default 16) and these sigmas (albedo,
normal, depth); rmse_guided is reported beside rmse and rmse_denoised, against the same reference,
with the guided kernel's time. --parent-denoise: the parent library filters its uniform frame too
(the plain filter's time on the commit before).
--atrous LEVELS SIGMA_L: the same frame also goes through rt_denoise_atrous with the feature buffers
(at --features SPP, default 16; the --guided sigmas, else the binding's) as edge stops; rmse_atrous,
the summed level kernels' time and the mean of the filter's stderr_out are reported beside the
others. --demodulate (with --atrous): it filters colour / albedo.
--cross R F K [SCALE]: the adaptive modes render through rt_render_adaptive_halves (the same frame and
error map) and the two half means go through rt_denoise_cross (variance_scale SCALE, default 2; the
--guided sigmas with the feature buffers if given); rmse_cross and the cross kernels' time are reported
beside the others, and the honesty of its error map: rms(stderr_out) over the RMSE of Y(out), linear,
against the same reference (atrous_honesty: rt_denoise_atrous's stderr_out by the same yardstick).

usage: python scripts/adaptive_bench.py --config C2 --thresholds 0.02 0.01 0.005 \
           [--parent lib/librtiow_parent.so] [--min-spp 64 --step-spp 64] [--denoise 10 3 0.45]
           [--features 16] [--guided 0.1 0.2 0.1] [--parent-denoise] [--atrous 5 4.0 [--demodulate]]
           [--cross 10 3 0.45 2.0]
           [--out adaptive_c2.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {   # bench.py's
    "C2": dict(scene=0, width=1200, height=800, spp=500, depth=50),
    "C3": dict(scene=5, width=800, height=800, spp=1000, depth=50),
    "C4": dict(scene=7, width=1920, height=1080, spp=1000, depth=50),
}

CHILD = r"""
import json, os, sys, time
sys.path.insert(0, {repo!r})
import numpy as np
import __graft_entry__ as ge
rt = ge.import_binding()
a = json.loads({args!r})
W, H, spp = a["width"], a["height"], a["spp"]
world = rt.World(1).build_scene(a["scene"])
cam, bg = rt.scene_camera(a["scene"], W, H)
r = rt.Renderer(0)
r.upload(world)
gamma = lambda x: np.sqrt(np.clip(x.astype(np.float64), 0.0, 0.999))
ref = ref_y = None
luma = lambda x: (lambda c: 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2])(x.astype(np.float64))
def honesty(out, se_out):   # rms(stderr_out) / RMSE of Y(out), linear
    return float(np.sqrt(np.mean(se_out ** 2)) / np.sqrt(np.mean((luma(out) - ref_y) ** 2)))
if a["ref"]:
    if not os.path.exists(a["ref"]):
        p = rt.Renderer.params(W, H, spp * a["ref_mult"], a["depth"], bg, 2, out_format=rt.RT_OUT_F32)
        np.save(a["ref"], r.render(cam, p))
    ref_y = luma(np.load(a["ref"]))
    ref = gamma(np.load(a["ref"]))
res = {{}}
dn = a.get("denoise")
ft, gd = a.get("features"), a.get("guided")
at = a.get("atrous")
cx = a.get("cross")
uniform_se = []
uniform_halves = []
guides = []
def features(d):
    pf = rt.Renderer.params(W, H, ft, a["depth"], bg, 1, out_format=rt.RT_OUT_F64)
    t0 = time.perf_counter()
    g = r.render_features(cam, pf)
    d["features_wall_ms"] = (time.perf_counter() - t0) * 1e3
    st = r.features_stats()
    d.update(features_ms=st.kernel_ms + st.reduce_ms, features_kernel_ms=st.kernel_ms, features_reduce_ms=st.reduce_ms,
             features_spp=ft)
    if not guides:
        guides.append(g)
def error_map(mode, se):
    if mode == "uniform":
        if not uniform_se:   # the same frame's error map: an adaptive call that never stops early
            p = rt.Renderer.params(W, H, spp, a["depth"], bg, 1, out_format=rt.RT_OUT_F32)
            uniform_se.append(r.render_adaptive(cam, p, a["min_spp"], a["step_spp"], 0.0)[3])
        se = uniform_se[0]
    return se
def atrous(mode, img, se, d):
    se = error_map(mode, se)
    t0 = time.perf_counter()
    out, se_out = r.denoise_atrous(img, se, *guides[0], gd or rt.GUIDE_SIGMAS, int(at[0]), float(at[1]), bool(a.get("demodulate")))
    d["atrous_wall_ms"] = (time.perf_counter() - t0) * 1e3
    st = r.atrous_stats()
    d.update(atrous_kernel_ms=st.kernel_ms, atrous_scratch_bytes=st.scratch_bytes, atrous_mean_stderr_out=float(se_out.mean()))
    if ref_y is not None:
        d["atrous_honesty"] = honesty(out, se_out)
    return out
def cross(mode, halves, se, d):
    se = error_map(mode, se)
    if mode == "uniform":
        if not uniform_halves:   # the same frame's halves: an adaptive call that never stops early
            p = rt.Renderer.params(W, H, spp, a["depth"], bg, 1, out_format=rt.RT_OUT_F32)
            uniform_halves.append(r.render_adaptive_halves(cam, p, a["min_spp"], a["step_spp"], 0.0)[4:])
        halves = uniform_halves[0]
    g = guides[0] if gd else (None, None, None)
    t0 = time.perf_counter()
    out, se_out = r.denoise_cross(halves[0], halves[1], se, *g, gd or rt.GUIDE_SIGMAS, int(cx[0]), int(cx[1]), float(cx[2]),
                                  float(cx[3]))
    d["cross_wall_ms"] = (time.perf_counter() - t0) * 1e3
    st = r.cross_stats()
    d.update(cross_kernel_ms=st.kernel_ms, cross_lds_bytes=st.lds_bytes, cross_scratch_bytes=st.scratch_bytes,
             cross_rms_stderr_out=float(np.sqrt(np.mean(se_out ** 2))))
    if ref_y is not None:
        d["cross_honesty"] = honesty(out, se_out)
    r.denoise_cross(halves[0], halves[1], se, *g, gd or rt.GUIDE_SIGMAS, int(cx[0]), int(cx[1]), float(cx[2]), float(cx[3]),
                    want_stderr=False)
    d["cross_kernel_ms_no_stderr"] = r.cross_stats().kernel_ms
    return out
def denoised(mode, img, se, d):
    se = error_map(mode, se)
    t0 = time.perf_counter()
    out = r.denoise(img, se, int(dn[0]), int(dn[1]), float(dn[2]))
    d["denoise_wall_ms"] = (time.perf_counter() - t0) * 1e3
    st = r.denoise_stats()
    d.update(denoise_kernel_ms=st.kernel_ms, denoise_lds_bytes=st.lds_bytes)
    if gd:
        t0 = time.perf_counter()
        out_g = r.denoise_guided(img, se, *guides[0], gd, int(dn[0]), int(dn[1]), float(dn[2]))
        d["guided_wall_ms"] = (time.perf_counter() - t0) * 1e3
        d["guided_kernel_ms"] = r.denoise_stats().kernel_ms
        return out, out_g
    return out, None
def run(mode):
    p = rt.Renderer.params(W, H, spp, a["depth"], bg, 1, out_format=rt.RT_OUT_F32)
    t0 = time.perf_counter()
    if mode == "uniform":
        img = r.render(cam, p)
        ms = (time.perf_counter() - t0) * 1e3
        st = r.stats()
        return img, None, None, dict(wall_ms=ms, trace_ms=st.kernel_ms, reduce_ms=st.reduce_ms, samples=st.samples,
                                     schedule=st.schedule, n_batches=st.n_batches)
    halves = None
    if cx:
        img, tile_spp, tile_err, se, *halves = r.render_adaptive_halves(cam, p, a["min_spp"], a["step_spp"], float(mode))
    else:
        img, tile_spp, tile_err, se = r.render_adaptive(cam, p, a["min_spp"], a["step_spp"], float(mode))
    ms = (time.perf_counter() - t0) * 1e3
    st = r.adaptive_stats()
    d = st.as_dict()
    d.update(wall_ms=ms, reduce_ms=st.moments_ms, samples=st.samples_traced, mean_tile_spp=float(tile_spp.mean()),
             tiles_at_max=int((tile_spp == spp).sum()), tiles_at_min=int((tile_spp == st.min_spp).sum()),
             tile_error_pct=[float(x) for x in np.percentile(tile_err, [5, 25, 50, 75, 95, 100])])
    d["halves"] = int(bool(cx))
    return img, se, halves, d
for mode in a["modes"]:
    img, se, halves, d = run(mode)             # warm-up: code objects, buffers
    if ft:
        features(d)
    if dn:
        denoised(mode, img, se, d)
    if at:
        atrous(mode, img, se, d)
    if cx:
        cross(mode, halves, se, d)
for _ in range(a["reps"]):
    for mode in a["modes"]:
        img, se, halves, d = run(mode)
        if ft:
            features(d)
        out, out_g = denoised(mode, img, se, d) if dn else (None, None)
        out_a = atrous(mode, img, se, d) if at else None
        out_x = cross(mode, halves, se, d) if cx else None
        e = res.setdefault(mode, dict(runs=[]))
        e["runs"].append(d)
        if ref is not None and "rmse" not in e:
            e["rmse"] = float(np.sqrt(np.mean((gamma(img) - ref) ** 2)))
            if dn:
                e["rmse_denoised"] = float(np.sqrt(np.mean((gamma(out) - ref) ** 2)))
            if out_g is not None:
                e["rmse_guided"] = float(np.sqrt(np.mean((gamma(out_g) - ref) ** 2)))
            if out_a is not None:
                e["rmse_atrous"] = float(np.sqrt(np.mean((gamma(out_a) - ref) ** 2)))
            if out_x is not None:
                e["rmse_cross"] = float(np.sqrt(np.mean((gamma(out_x) - ref) ** 2)))
print("RESULT", json.dumps(res))
print("BUILD", rt.build_info())
"""


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2", choices=sorted(CONFIGS))
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.0])
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--step-spp", type=int, default=64)
    ap.add_argument("--parent", default=None, help="a library built from the parent commit (uniform mode only)")
    ap.add_argument("--lib", default=os.path.join("rust-ray-tracing-in-a-weekend_amd", "lib", "librtiow_amd.so"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ref-mult", type=int, default=4, help="the error reference: uniform at this many x spp (0: none)")
    ap.add_argument("--denoise", type=float, nargs=3, default=None, metavar=("R", "F", "K"),
                    help="also filter every frame with rt_denoise: radius, patch, k")
    ap.add_argument("--features", type=int, default=None, metavar="SPP",
                    help="also time rt_render_features at SPP samples per pixel")
    ap.add_argument("--guided", type=float, nargs=3, default=None, metavar=("SA", "SN", "SZ"),
                    help="with --denoise: also filter with rt_denoise_guided (sigmas of albedo, normal, depth)")
    ap.add_argument("--parent-denoise", action="store_true", help="the parent library runs the plain filter too")
    ap.add_argument("--atrous", type=float, nargs=2, default=None, metavar=("LEVELS", "SIGMA_L"),
                    help="also filter every frame with rt_denoise_atrous (guided by the feature buffers)")
    ap.add_argument("--demodulate", action="store_true", help="with --atrous: filter colour / albedo")
    ap.add_argument("--cross", type=float, nargs="+", default=None, metavar="R F K [SCALE]",
                    help="also filter the two half frames of every mode with rt_denoise_cross")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.cross:
        if len(a.cross) not in (3, 4):
            ap.error("--cross takes R F K [SCALE]")
        a.cross = list(a.cross) + [2.0] * (4 - len(a.cross))
    if a.guided and not a.denoise:
        ap.error("--guided needs --denoise R F K")
    if a.demodulate and not a.atrous:
        ap.error("--demodulate needs --atrous LEVELS SIGMA_L")
    if (a.guided or a.atrous) and not a.features:   # (--cross alone runs unguided)
        a.features = 16
    cfg = CONFIGS[a.config]
    tmp = tempfile.TemporaryDirectory()   # the error reference: rendered by the first child, read by the others
    ref = os.path.join(tmp.name, f"adaptive_ref_{a.config}_x{a.ref_mult}.npy") if a.ref_mult > 0 else None
    jobs = [("new", a.lib, ["uniform"] + [repr(t) for t in a.thresholds])]
    if a.parent:
        jobs.insert(0, ("parent", a.parent, ["uniform"]))
    runs, builds = {}, {}
    for _ in range(a.rounds):
        for name, lib, modes in jobs:
            args = dict(cfg, modes=modes, reps=a.reps, min_spp=a.min_spp, step_spp=a.step_spp, ref=ref,
                        ref_mult=a.ref_mult)
            if a.denoise and (name == "new" or a.parent_denoise):
                args["denoise"] = a.denoise
            if name == "new":
                args.update(features=a.features, guided=a.guided, atrous=a.atrous, demodulate=a.demodulate, cross=a.cross)
            env = dict(os.environ, RT_LIB_PATH=os.path.abspath(os.path.join(REPO, lib)))
            out = subprocess.run([sys.executable, "-c", CHILD.format(repo=REPO, args=json.dumps(args))], env=env,
                                 capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                print(f"{name}: child failed ({out.returncode})\n{out.stderr[-2000:]}")
                sys.exit(out.returncode if out.returncode > 0 else 1)
            d = json.loads([x for x in out.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
            if name not in builds:   # rt_build_info of each library, once
                builds[name] = [x for x in out.stdout.splitlines() if x.startswith("BUILD ")][-1][6:]
                print(f"  {name}: rt_build_info {builds[name]}", flush=True)
            for mode, e in d.items():
                k = runs.setdefault(f"{name}:{mode}", dict(runs=[], rmse=e.get("rmse"), rmse_denoised=e.get("rmse_denoised"),
                                                           rmse_guided=e.get("rmse_guided"), rmse_atrous=e.get("rmse_atrous"),
                                                           rmse_cross=e.get("rmse_cross")))
                k["runs"] += e["runs"]
                print(f"  {name}:{mode}: wall {['%.2f' % x['wall_ms'] for x in e['runs']]}", flush=True)
    uniform_px = cfg["width"] * cfg["height"] * cfg["spp"]
    base = median([x["wall_ms"] for x in runs[("parent" if a.parent else "new") + ":uniform"]["runs"]])
    summary = {}
    for key, e in runs.items():
        rs = e["runs"]
        wall = [x["wall_ms"] for x in rs]
        red = median([x["reduce_ms"] for x in rs])
        s = dict(wall_ms_median=median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall), n=len(wall),
                 wall_over_base=median(wall) / base, trace_ms=median([x["trace_ms"] for x in rs]), reduce_ms=red,
                 samples=rs[0]["samples"], samples_over_uniform=rs[0]["samples"] / uniform_px,
                 reduce_GBps=rs[0]["samples"] * 24 / red / 1e6 if red > 0 else None, rmse=e["rmse"])
        if "tile_error_pct" in rs[0]:
            s["tile_error_pct_5_25_50_75_95_100"] = rs[0]["tile_error_pct"]
        if "denoise_kernel_ms" in rs[0]:
            s.update(rmse_denoised=e["rmse_denoised"], denoise_kernel_ms=median([x["denoise_kernel_ms"] for x in rs]),
                     denoise_kernel_ms_min=min(x["denoise_kernel_ms"] for x in rs),
                     denoise_kernel_ms_max=max(x["denoise_kernel_ms"] for x in rs),
                     denoise_wall_ms=median([x["denoise_wall_ms"] for x in rs]), denoise_lds_bytes=rs[0]["denoise_lds_bytes"],
                     denoise_kernel_over_wall=median([x["denoise_kernel_ms"] for x in rs]) / median(wall))
        if "features_ms" in rs[0]:
            s.update(features_spp=rs[0]["features_spp"], features_ms=median([x["features_ms"] for x in rs]),
                     features_kernel_ms=median([x["features_kernel_ms"] for x in rs]),
                     features_reduce_ms=median([x["features_reduce_ms"] for x in rs]),
                     features_wall_ms=median([x["features_wall_ms"] for x in rs]))
        if "guided_kernel_ms" in rs[0]:
            s.update(rmse_guided=e["rmse_guided"], guided_kernel_ms=median([x["guided_kernel_ms"] for x in rs]),
                     guided_wall_ms=median([x["guided_wall_ms"] for x in rs]), guided_sigmas=a.guided)
        if "atrous_kernel_ms" in rs[0]:
            s.update(rmse_atrous=e["rmse_atrous"], atrous_kernel_ms=median([x["atrous_kernel_ms"] for x in rs]),
                     atrous_kernel_ms_min=min(x["atrous_kernel_ms"] for x in rs),
                     atrous_kernel_ms_max=max(x["atrous_kernel_ms"] for x in rs),
                     atrous_wall_ms=median([x["atrous_wall_ms"] for x in rs]), atrous=a.atrous, demodulate=int(a.demodulate),
                     atrous_scratch_bytes=rs[0]["atrous_scratch_bytes"],
                     atrous_mean_stderr_out=median([x["atrous_mean_stderr_out"] for x in rs]))
        if "atrous_honesty" in rs[0]:
            s["atrous_honesty"] = rs[0]["atrous_honesty"]
        if "cross_kernel_ms" in rs[0]:
            s.update(rmse_cross=e["rmse_cross"], cross=a.cross, cross_kernel_ms=median([x["cross_kernel_ms"] for x in rs]),
                     cross_kernel_ms_min=min(x["cross_kernel_ms"] for x in rs),
                     cross_kernel_ms_max=max(x["cross_kernel_ms"] for x in rs),
                     cross_kernel_ms_no_stderr=median([x["cross_kernel_ms_no_stderr"] for x in rs]),
                     cross_wall_ms=median([x["cross_wall_ms"] for x in rs]), cross_lds_bytes=rs[0]["cross_lds_bytes"],
                     cross_scratch_bytes=rs[0]["cross_scratch_bytes"], cross_rms_stderr_out=rs[0]["cross_rms_stderr_out"],
                     cross_honesty=rs[0].get("cross_honesty"), halves=rs[0].get("halves"))
        for k in ("passes", "classify_ms", "mean_tile_spp", "tiles_at_max", "tiles_at_min", "tiles", "schedule", "n_batches",
                  "max_pass_batches"):
            if k in rs[0]:
                s[k] = median([x[k] for x in rs])
        summary[key] = s
        print(f"{a.config} {key}: " + json.dumps(s))
    if a.out:
        doc = dict(config=a.config, params=cfg, min_spp=a.min_spp, step_spp=a.step_spp, base_wall_ms=base, results=summary)
        if a.denoise:
            doc["denoise"] = a.denoise
        if a.features:
            doc["features_spp"] = a.features
        if a.guided:
            doc["guided"] = a.guided
        if a.atrous:
            doc.update(atrous=a.atrous, demodulate=int(a.demodulate))
        if a.cross:
            doc["cross"] = a.cross
        json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
