"""What owns a context's device resources: destroying a context with work still in flight on a
caller's stream, and reading each timed span (rt_last_stats, rt_features_last_stats,
rt_denoise_last_stats, rt_atrous_last_stats) exactly once.

Scene 0 at 48 x 32, 4 spp, f64; the a-trous filter at 3 levels (two state buffers of scratch)
without guides, over the render's frame and a fixed error map.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, SPP, LEVELS = 48, 32, 4, 3


def _context(rt):
    r = rt.Renderer(0)
    r.upload(rt.World(1).build_scene(0))
    cam, bg = rt.scene_camera(0, W, H)
    return r, cam, rt.Renderer.params(W, H, SPP, 50, bg, 1, out_format=rt.RT_OUT_F64)


def _error_map():
    y, x = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(0.02 + 0.01 * ((x + 2 * y) % 5), dtype=np.float64)


def test_destroy_with_work_in_flight_then_reuse(rt):
    import torch
    se = _error_map()
    ref, cam, p = _context(rt)
    try:
        want = ref.render(cam, p)
        want_out, want_se = ref.denoise_atrous(want, se, levels=LEVELS)
    finally:
        ref.close()

    f64 = dict(dtype=torch.float64, device="cuda:0")
    se_d = torch.from_numpy(se).to("cuda:0")
    for cycle in range(3):
        frame_d, out_d = torch.full((H, W, 3), 7.0, **f64), torch.full((H, W, 3), 7.0, **f64)
        se_out_d = torch.full((H, W), 7.0, **f64)
        torch.cuda.synchronize()
        stream = torch.cuda.Stream(torch.device("cuda", 0))
        own, cam, p = _context(rt)
        try:
            own.render_device(cam, p, frame_d.data_ptr(), stream=stream.cuda_stream)
            own.denoise_atrous_device(frame_d.data_ptr(), se_d.data_ptr(), out_d.data_ptr(), W, H,
                                      out_format=rt.RT_OUT_F64, levels=LEVELS, stderr_out_ptr=se_out_d.data_ptr(),
                                      stream=stream.cuda_stream)
        finally:
            own.close()           # no synchronisation before it: the context waits for its own work
        again, cam, p = _context(rt)
        try:
            got = again.render(cam, p)
            got_out, got_se = again.denoise_atrous(got, se, levels=LEVELS)
        finally:
            again.close()
        assert np.array_equal(got, want), cycle
        assert np.array_equal(got_out, want_out) and np.array_equal(got_se, want_se), cycle
        # and what the destroyed context had enqueued ran to its end on intact buffers
        torch.cuda.synchronize()
        assert np.array_equal(frame_d.cpu().numpy(), want), cycle
        assert np.array_equal(out_d.cpu().numpy(), want_out) and np.array_equal(se_out_d.cpu().numpy(), want_se), cycle


def test_every_timed_span_resolves_once(rt):
    import torch
    getters = {"rt_last_stats": ("stats", ("kernel_ms", "reduce_ms")),
               "rt_features_last_stats": ("features_stats", ("kernel_ms", "reduce_ms")),
               "rt_denoise_last_stats": ("denoise_stats", ("kernel_ms",)),
               "rt_atrous_last_stats": ("atrous_stats", ("kernel_ms",))}
    fresh = rt.Renderer(0)
    try:
        for name, (getter, _) in getters.items():     # nothing enqueued yet: zeros (and RT_OK: no RTError)
            s = getattr(fresh, getter)()
            assert bytes(s) == bytes(len(bytes(s))), name
    finally:
        fresh.close()

    own, cam, p = _context(rt)
    try:
        f64 = dict(dtype=torch.float64, device="cuda:0")
        frame_d, out_d, out2_d = (torch.zeros((H, W, 3), **f64) for _ in range(3))
        a_d, n_d = torch.zeros((H, W, 3), **f64), torch.zeros((H, W, 3), **f64)
        z_d, se_d = torch.zeros((H, W), **f64), torch.from_numpy(_error_map()).to("cuda:0")
        torch.cuda.synchronize()
        s = torch.cuda.Stream(torch.device("cuda", 0)).cuda_stream
        own.render_device(cam, p, frame_d.data_ptr(), stream=s)
        own.render_features_device(cam, p, a_d.data_ptr(), n_d.data_ptr(), z_d.data_ptr(), stream=s)
        own.denoise_device(frame_d.data_ptr(), se_d.data_ptr(), out_d.data_ptr(), W, H, rt.RT_OUT_F64, 5, 2, 1.0, stream=s)
        own.denoise_atrous_device(frame_d.data_ptr(), se_d.data_ptr(), out2_d.data_ptr(), W, H, out_format=rt.RT_OUT_F64,
                                  levels=LEVELS, stream=s)
        for name, (getter, times) in getters.items():
            first = getattr(own, getter)()            # waits for the span's last event
            for t in times:
                ms = getattr(first, t)
                print(f"{name}.{t} = {ms:.4f} ms")
                assert math.isfinite(ms) and ms >= 0.0, (name, t, ms)
            second = getattr(own, getter)()
            assert bytes(second) == bytes(first), name
        torch.cuda.synchronize()
    finally:
        own.close()
