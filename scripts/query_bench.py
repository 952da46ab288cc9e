#!/usr/bin/env python3
"""What rt_trace_rays costs per ray, against the kernel that casts the same rays itself
(DESIGN.md 5.15).

The random scene at 1200x800, the primary rays of sample 0 (rt_camera_rays), on one context:

  closest tiled     RT_QUERY_CLOSEST, rays in 8x8 tile order (the chunk kernels' lane order)
  closest rows      the same rays row-major
  closest shuffled  the same rays in a seeded shuffle (reported, not gated)
  any tiled         RT_QUERY_ANY, tile order, t_max = inf
  any half          RT_QUERY_ANY, tile order, t_max = half each ray's closest t (nothing is occluded)
  features spp 1    rt_render_features at spp 1: the yardstick, which makes these rays itself
  final tiled       RT_QUERY_CLOSEST over the final scene's primary rays, tile order
  final features    rt_render_features at spp 1 on the final scene

Rays and results live in device memory (torch tensors) and every call is a device-pointer call, so a
line is the kernel alone: HIP-event milliseconds (rt_query_stats.kernel_ms, features_stats().kernel_ms)
and Mrays/s from them. Each line runs `--reps` times after one warm-up, the lines interleaved, and
is printed once per run; pass --log to append the lines to a file.

usage: python scripts/query_bench.py [--width 1200 --height 800] [--reps 3] [--log profiles/query_c2.log]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1200)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    rt = ge.import_binding()
    W, H, n = a.width, a.height, a.width * a.height
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)

    def upload(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    scenes = {}
    for name, scene_id in (("random", 0), ("final", 7)):
        cam, bg = rt.scene_camera(scene_id, W, H)
        r = rt.Renderer(0)
        r.upload(rt.World(1).build_scene(scene_id, rt.load_earth_texture() if scene_id in rt.SCENES_NEEDING_IMAGE else None))
        tiled = rt.camera_rays(cam, W, H, a.seed, 0, tiled=True)
        scenes[name] = dict(r=r, cam=cam, bg=bg, tiled=tiled, bound=float(np.abs(tiled["o"]).max()))
    S = scenes["random"]
    rows = rt.camera_rays(S["cam"], W, H, a.seed, 0)
    shuffled = rows[np.random.default_rng(7).permutation(n)]
    closest_t = S["r"].trace_rays(S["tiled"], seed=a.seed)["t"]
    half = S["tiled"].copy()
    half["t_max"] = np.where(np.isfinite(closest_t), 0.5 * closest_t, 1.0)
    d_hits = torch.empty(n * 80, dtype=torch.uint8, device=dev)
    d_occ = torch.empty(n, dtype=torch.uint8, device=dev)
    d_feat = [torch.empty((H, W, 3), dtype=torch.float64, device=dev) for _ in range(2)] + \
             [torch.empty((H, W), dtype=torch.float64, device=dev)]
    sets = {k: upload(v) for k, v in (("tiled", S["tiled"]), ("rows", rows), ("shuffled", shuffled), ("half", half),
                                      ("final", scenes["final"]["tiled"]))}
    torch.cuda.synchronize()

    def query(scene, rays, mode):
        sc = scenes[scene]
        out = dict(occluded_ptr=d_occ.data_ptr()) if mode == rt.RT_QUERY_ANY else dict(hits_ptr=d_hits.data_ptr())
        sc["r"].trace_rays_device(sets[rays].data_ptr(), n, mode, seed=a.seed, origin_bound=sc["bound"],
                                  stream=stream.cuda_stream, **out)
        st = sc["r"].query_stats()
        return dict(kernel_ms=st.kernel_ms, slab32=st.slab32, variant=st.variant_features)

    def features(scene):
        sc = scenes[scene]
        p = rt.Renderer.params(W, H, 1, 50, sc["bg"], a.seed, out_format=rt.RT_OUT_F64)
        sc["r"].render_features_device(sc["cam"], p, *(t.data_ptr() for t in d_feat), stream=stream.cuda_stream)
        st = sc["r"].features_stats()
        return dict(kernel_ms=st.kernel_ms, variant=st.variant_features)

    lines = [("closest tiled", lambda: query("random", "tiled", rt.RT_QUERY_CLOSEST)),
             ("closest rows", lambda: query("random", "rows", rt.RT_QUERY_CLOSEST)),
             ("closest shuffled", lambda: query("random", "shuffled", rt.RT_QUERY_CLOSEST)),
             ("any tiled", lambda: query("random", "tiled", rt.RT_QUERY_ANY)),
             ("any half", lambda: query("random", "half", rt.RT_QUERY_ANY)),
             ("features spp 1", lambda: features("random")),
             ("final tiled", lambda: query("final", "final", rt.RT_QUERY_CLOSEST)),
             ("final features", lambda: features("final"))]
    for _, fn in lines:   # warm-up: code objects, buffers
        fn()
    out = [f"query_bench {W}x{H} sample 0, {n} rays; rt_build_info {rt.build_info()}"]
    for rep in range(a.reps):
        for name, fn in lines:
            d = fn()
            d.update(run=rep, mrays_per_s=round(n / d["kernel_ms"] / 1e3, 1), kernel_ms=round(d["kernel_ms"], 4))
            out.append(f"{name}: " + json.dumps(d))
    stream.synchronize()
    occluded_half = int(d_occ.cpu().numpy().sum())   # (the last ANY call was "any half")
    out.append(f"any half: occluded {occluded_half} of {n}; closest tiled: hits {int(np.isfinite(closest_t).sum())} of {n}")
    print("\n".join(out))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "a") as f:
            f.write("\n".join(out) + "\n")
    for sc in scenes.values():
        sc["r"].close()


if __name__ == "__main__":
    main()
