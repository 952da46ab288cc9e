"""rt_render_features on the device: first-hit albedo, normal and depth (include/rt/rt_abi.h).

Albedo against the oracle: every world is built through tests/features_reference.py's LightTwin,
whose oracle side renders at max_depth = 1 exactly the albedo buffer (the same primary rays, the
same chunked sum); bar as in tests/test_gpu_parity.py (L_inf <= 1e-3 and 1e-9 relative). One world
per kernel variant. Normal, depth and albedo against the numpy first-hit restatement of the same
module on worlds of spheres and rects (1e-9 absolute plus relative, no pixel excluded). Then what
must not change the bits: the acceleration structure, a larger kernel variant, the chunk size where
the boundaries coincide, a repeat, leaving outputs out, device pointers.
"""
import ctypes

import numpy as np
import pytest

from tests import features_reference as fr
from tests import oracle_binding as ob
from tests import test_gpu_nesting as nesting
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

BG = (0.5, 0.6, 0.8)
#         W,  H, spp, spp_chunk
SHAPES = [(48, 32, 6, 0), (37, 21, 17, 4), (9, 5, 1, 0)]   # whole tiles; ragged edge tiles and a ragged last chunk; one tile


def _spheres_world(rt):
    """Checker ground, moving spheres (shutter [0, 1]), metal and glass: the spheres variant."""
    tw = fr.LightTwin(rt, 3)
    ground = tw.lambertian(tw.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    red = tw.lambertian(tw.solid(0.7, 0.1, 0.1))
    metal = tw.metal((0.8, 0.6, 0.2), 0.2)
    glass = tw.dielectric(1.5)
    tw.push(tw.sphere(ground, (0.0, -1000.0, 0.0), 1000.0))
    for i in range(5):
        c0 = (-2.0 + i, 0.3, 0.2 * i)
        tw.push(tw.moving_sphere((red, metal, glass)[i % 3], c0, (c0[0], c0[1] + 0.4, c0[2]), 0.0, 1.0, 0.3))
    tw.push(tw.sphere(glass, (0.5, 1.2, -1.0), 0.4))
    tw.push(tw.sphere(metal, (-1.5, 0.9, 1.0), 0.5))
    return tw, ((6.0, 2.0, 5.0), (0.0, 0.5, 0.0), 40.0)


def _cornell_world(rt, media: bool, density: float = 0.01):
    """A Cornell-like box seen from far enough that rays pass beside it, with two rotated and
    translated boxes, or (media) the two boxes as constant media of the given density."""
    tw = fr.LightTwin(rt, 7)
    red = tw.lambertian(tw.solid(0.65, 0.05, 0.05))
    white = tw.lambertian(tw.solid(0.73, 0.73, 0.73))
    green = tw.lambertian(tw.solid(0.12, 0.45, 0.15))
    light = tw.diffuse_light(tw.solid(7.0, 7.0, 7.0))
    tw.push(tw.yz_rect(green, 0.0, 555.0, 0.0, 555.0, 555.0))
    tw.push(tw.yz_rect(red, 0.0, 555.0, 0.0, 555.0, 0.0))
    tw.push(tw.xz_rect(light, 113.0, 443.0, 127.0, 432.0, 554.0))
    tw.push(tw.xz_rect(white, 0.0, 555.0, 0.0, 555.0, 0.0))
    tw.push(tw.xz_rect(white, 0.0, 555.0, 0.0, 555.0, 555.0))
    tw.push(tw.xy_rect(white, 0.0, 555.0, 0.0, 555.0, 555.0))
    metal = tw.metal((0.8, 0.85, 0.88), 0.0)
    b1 = tw.translate(tw.rotate_y(tw.box((0.0, 0.0, 0.0), (165.0, 330.0, 165.0), white if media else metal), 15.0),
                      (265.0, 0.0, 295.0))
    b2 = tw.translate(tw.rotate_y(tw.box((0.0, 0.0, 0.0), (165.0, 165.0, 165.0), white), -18.0), (130.0, 0.0, 65.0))
    if media:
        tw.push(tw.constant_medium(b1, density, tw.isotropic(tw.solid(0.1, 0.1, 0.1))))
        tw.push(tw.constant_medium(b2, density, tw.isotropic(tw.solid(0.9, 0.9, 0.9))))
    else:
        tw.push(b1)
        tw.push(b2)
    return tw, ((278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 55.0)


def _final_world(rt, density: float = 1.5):
    """Top-level rects, a Perlin sphere, a sphere-bounded medium (of the given density) and a
    translated, rotated BVH of spheres: the final-scene variant."""
    tw = fr.LightTwin(rt, 11)
    ground = tw.lambertian(tw.solid(0.48, 0.83, 0.53))
    white = tw.lambertian(tw.solid(0.73, 0.73, 0.73))
    light = tw.diffuse_light(tw.solid(7.0, 7.0, 7.0))
    tw.push(tw.xz_rect(ground, -6.0, 6.0, -6.0, 6.0, 0.0))
    tw.push(tw.xz_rect(light, -1.0, 1.0, -1.0, 1.0, 4.0))
    tw.push(tw.xy_rect(white, -3.0, 3.0, 0.0, 2.5, -4.0))
    tw.push(tw.sphere(tw.lambertian(tw.noise(4.0)), (-1.6, 0.8, 0.5), 0.8))
    tw.push(tw.constant_medium(tw.sphere(tw.dielectric(1.5), (1.5, 0.7, 1.0), 0.7), density, tw.isotropic(tw.solid(0.2, 0.4, 0.9))))
    balls = tw.bvh([tw.sphere(white, (0.35 * (i % 5), 0.2 + 0.35 * (i // 5), 0.1 * (i % 3)), 0.15) for i in range(15)])
    tw.push(tw.translate(tw.rotate_y(balls, 15.0), (-0.6, 0.0, -1.8)))
    return tw, ((5.0, 3.0, 8.0), (0.0, 0.8, 0.0), 40.0)


def _nested_world(rt, monkeypatch):
    """tests/test_gpu_nesting.py's nested world, its constructor calls issued to a LightTwin."""
    monkeypatch.setattr(ob, "TwinWorld", fr.LightTwin)
    return nesting._nested_world(rt), ((7.0, 4.0, 9.0), (0.0, 0.7, 0.0), 40.0)


WORLDS = {"spheres": (0, lambda rt, mp: _spheres_world(rt)),
          "rectinst": (35, lambda rt, mp: _cornell_world(rt, False)),
          "media": (103, lambda rt, mp: _cornell_world(rt, True)),
          "final": (287, lambda rt, mp: _final_world(rt)),
          "all": (4095, _nested_world)}
_built = {}


def _world(rt, monkeypatch, name):
    if name not in _built:
        _built[name] = WORLDS[name][1](rt, monkeypatch)
    return _built[name]


def _camera(rt, view, W, H, aperture=0.1):
    look_from, look_at, vfov = view
    return rt.camera_new(look_from, look_at, (0.0, 1.0, 0.0), vfov, W / H, aperture, 10.0, 0.0, 1.0)


def _params(rt, W, H, spp, chunk=0, **kw):
    return rt.Renderer.params(W, H, spp, 50, BG, 1, spp_chunk=chunk, out_format=rt.RT_OUT_F64, **kw)


@pytest.mark.parametrize("W,H,spp,chunk", SHAPES)
@pytest.mark.parametrize("name", list(WORLDS))
def test_albedo_matches_the_oracle_light_twin(rt, renderer, monkeypatch, name, W, H, spp, chunk):
    tw, view = _world(rt, monkeypatch, name)
    cam = _camera(rt, view, W, H)
    renderer.upload(tw.product)
    albedo, normal, depth = renderer.render_features(cam, _params(rt, W, H, spp, chunk))
    st = renderer.features_stats()
    assert st.variant_features == WORLDS[name][0]
    assert st.samples == W * H * spp and st.kernel_ms > 0 and st.spp_chunk == (chunk or 1)
    ref = tw.oracle.render(fr.cam24(cam), BG, W, H, spp, max_depth=1, spp_chunk=chunk)
    if (W, H) == SHAPES[0][:2]:   # the world shows hits and misses
        miss = np.abs(ref - np.array(BG)).max(-1) < 1e-12
        assert 0 < int(miss.sum()) < W * H, int(miss.sum())
        assert (np.abs(ref - np.array(BG)).max(-1) > 1e-3).sum() > W * H // 8
    assert_parity(albedo, ref, f"albedo, {name} {W}x{H}x{spp}")
    # a miss has neither normal nor depth; a pixel with a hit has both
    assert np.isfinite(normal).all() and np.isfinite(depth).all() and (depth >= 0).all()
    assert np.array_equal(depth == 0, (normal == 0).all(-1) & (depth == 0))
    assert (np.linalg.norm(normal, axis=-1) <= 1 + 1e-12).all()


SIMPLE = {
    "spheres": ([("sphere", (0.0, -100.5, -1.0), 100.0, (0.8, 0.8, 0.0)), ("sphere", (0.0, 0.0, -1.0), 0.5, (0.1, 0.2, 0.5)),
                 ("sphere", (-1.0, 0.0, -1.0), 0.5, (1.0, 1.0, 1.0)), ("sphere", (1.0, 0.0, -1.0), 0.5, (0.8, 0.6, 0.2)),
                 ("sphere", (0.3, 0.9, -1.6), 0.4, (0.3, 0.7, 0.3))],
                ["lambertian", "lambertian", "dielectric", "metal", "lambertian"], 0),
    "spheres_rects": ([("rect", 1, -3.0, 3.0, -4.0, 1.0, -0.5, (0.5, 0.5, 0.4)), ("rect", 0, -1.5, 1.5, -0.5, 1.5, -2.5, (0.2, 0.3, 0.9)),
                       ("rect", 2, -0.5, 1.0, -2.5, -0.5, -1.5, (4.0, 3.0, 2.0)), ("sphere", (0.0, 0.0, -1.0), 0.5, (0.7, 0.2, 0.1)),
                       ("sphere", (0.9, 0.1, -1.4), 0.6, (1.0, 1.0, 1.0))],
                      ["lambertian", "metal", "light", "lambertian", "dielectric"], 35),
}


@pytest.mark.parametrize("W,H,spp", [(37, 21, 5), (9, 5, 2)])
@pytest.mark.parametrize("name", list(SIMPLE))
def test_normal_depth_albedo_match_the_numpy_first_hit(rt, renderer, name, W, H, spp):
    prims, mats, variant = SIMPLE[name]
    cam = _camera(rt, ((0.0, 0.6, 2.0), (0.0, 0.1, -1.0), 60.0), W, H, aperture=0.0)
    renderer.upload(fr.build_simple(rt, prims, mats))
    albedo, normal, depth = renderer.render_features(cam, _params(rt, W, H, spp))
    assert renderer.features_stats().variant_features == variant
    ra, rn, rd, hits = fr.first_hit(prims, cam, BG, W, H, spp)
    assert (hits == 0).any() and (hits == spp).any()
    for got, ref, what in ((albedo, ra, "albedo"), (normal, rn, "normal"), (depth, rd, "depth")):
        err = float(np.max(np.abs(got - ref) / (1e-9 + 1e-9 * np.abs(ref))))
        print(f"{name} {W}x{H}x{spp} {what}: max |got - ref| / (1e-9 + 1e-9 |ref|) = {err:.3e}")
        assert err <= 1.0, what
    assert (np.linalg.norm(normal, axis=-1) <= 1 + 1e-12).all()
    none = hits == 0
    assert (depth[none] == 0).all() and (normal[none] == 0).all() and (depth[~none] > 0).all()


def _all7(r, cam, p):
    a, n, d = r.render_features(cam, p)
    return np.concatenate([a, n, d[..., None]], axis=-1)


def test_bits_do_not_depend_on_the_acceleration_structure(rt, renderer, monkeypatch):
    tw, view = _world(rt, monkeypatch, "all")
    W, H, spp = 32, 24, 4
    cam = _camera(rt, view, W, H)
    frames = []
    for accel in (rt.RT_ACCEL_SAH, rt.RT_ACCEL_LINEAR, rt.RT_ACCEL_MEDIAN):
        renderer.upload(tw.product, accel)
        frames.append(_all7(renderer, cam, _params(rt, W, H, spp)))
    assert np.array_equal(frames[1], frames[0]) and np.array_equal(frames[2], frames[0])
    assert (frames[0][..., 6] > 0).any()


def test_bits_do_not_depend_on_the_kernel_variant(rt, renderer, monkeypatch):
    tw, view = _world(rt, monkeypatch, "spheres")
    W, H, spp = 37, 21, 6
    cam = _camera(rt, view, W, H)
    renderer.upload(tw.product)
    want = _all7(renderer, cam, _params(rt, W, H, spp))
    assert renderer.features_stats().variant_features == 0
    r = rt.Renderer(0)
    try:
        r.set_option(rt.RT_OPT_EXTRA_FEATURES, 4095)
        r.upload(tw.product)
        got = _all7(r, cam, _params(rt, W, H, spp))
        assert r.features_stats().variant_features == 4095
    finally:
        r.close()
    assert np.array_equal(got, want)


def test_chunk_repeat_and_null_outputs(rt, renderer, monkeypatch):
    tw, view = _world(rt, monkeypatch, "final")
    W, H = 37, 21
    cam = _camera(rt, view, W, H)
    renderer.upload(tw.product)
    # one chunk of 6 either way (spp_chunk is cut at spp)
    one = _all7(renderer, cam, _params(rt, W, H, 6, 6))
    assert np.array_equal(_all7(renderer, cam, _params(rt, W, H, 6, 9)), one)
    # spp 20: the automatic chunk is 2
    auto = _all7(renderer, cam, _params(rt, W, H, 20, 0))
    assert renderer.features_stats().spp_chunk == 2
    assert np.array_equal(_all7(renderer, cam, _params(rt, W, H, 20, 2)), auto)
    assert np.array_equal(_all7(renderer, cam, _params(rt, W, H, 20, 0)), auto)          # a repeat call
    for keep in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        a, n, d = renderer.render_features(cam, _params(rt, W, H, 20, 0), *(bool(k) for k in keep))
        assert [x is not None for x in (a, n, d)] == [bool(k) for k in keep]
        assert a is None or np.array_equal(a, auto[..., 0:3])
        assert n is None or np.array_equal(n, auto[..., 3:6])
        assert d is None or np.array_equal(d, auto[..., 6])


def test_buffer_batches_keep_the_bits(rt, renderer, monkeypatch):
    """96x64 at 8 spp in chunks of 1: a chunk's partials are 6144 x 56 B = 336 KiB, so a trace-output
    bound of 1 MiB (the option's minimum) holds 3 chunks and the call takes 3 batches (3 + 3 + 2
    chunks), the running sums carried between them; the default bound takes one. Same bits."""
    tw, view = _world(rt, monkeypatch, "spheres")
    W, H, spp = 96, 64, 8
    cam = _camera(rt, view, W, H)
    renderer.upload(tw.product)
    want = _all7(renderer, cam, _params(rt, W, H, spp, 1))
    r = rt.Renderer(0)
    try:
        r.set_option(rt.RT_OPT_TRACE_BUF_BYTES, 1 << 20)
        assert r.get_option(rt.RT_OPT_TRACE_BUF_BYTES) == 1 << 20
        r.upload(tw.product)
        got = _all7(r, cam, _params(rt, W, H, spp, 1))
    finally:
        r.close()
    assert np.array_equal(got, want)


def test_device_pointer_path_is_the_host_pointer_path(rt, renderer, monkeypatch):
    import torch
    tw, view = _world(rt, monkeypatch, "media")
    W, H, spp = 37, 21, 17
    cam = _camera(rt, view, W, H)
    renderer.upload(tw.product)
    want = renderer.render_features(cam, _params(rt, W, H, spp, 4))
    a, n = (torch.full((H, W, 3), 7.0, dtype=torch.float64, device="cuda:0") for _ in range(2))
    d = torch.full((H, W), 7.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    renderer.render_features_device(cam, _params(rt, W, H, spp, 4), a.data_ptr(), n.data_ptr(), d.data_ptr(),
                                    stream=stream.cuda_stream)
    assert renderer.features_stats().kernel_ms > 0       # waits for the kernels
    stream.synchronize()
    for got, ref in zip((a, n, d), want):
        assert np.array_equal(got.cpu().numpy(), ref)


def test_errors_leave_the_context_rendering(rt, renderer, monkeypatch):
    tw, view = _world(rt, monkeypatch, "spheres")
    W, H, spp = 24, 16, 4
    cam = _camera(rt, view, W, H)
    renderer.upload(tw.product)
    p_render = rt.Renderer.params(W, H, spp, 50, BG, 1, out_format=rt.RT_OUT_F64)
    before = renderer.render(cam, p_render).copy()
    lib = rt.load_library()
    bufs = [np.empty((H, W, 3)), np.empty((H, W, 3)), np.empty((H, W))]
    out = rt.FeaturesOut(*(b.ctypes.data for b in bufs))

    def call(h, params, o):
        return rt.ERRORS.get(lib.rt_render_features(h, ctypes.byref(cam), ctypes.byref(params), ctypes.byref(o)))

    assert lib.rt_render_features(renderer.h, ctypes.byref(cam), ctypes.byref(_params(rt, W, H, spp)), ctypes.byref(out)) == rt.RT_OK
    for kw in (dict(row_begin=1), dict(row_stride=2), dict(row_block=2), dict(tile_shard=1)):
        assert call(renderer.h, _params(rt, W, H, spp, **kw), out) == "RT_ERR_INVALID", kw
        assert lib.rt_last_error()
    assert call(renderer.h, _params(rt, W, H, 0), out) == "RT_ERR_INVALID"
    assert call(renderer.h, _params(rt, W, H, spp), rt.FeaturesOut(None, None, None)) == "RT_ERR_INVALID"
    renderer.set_precision(rt.RT_PREC_F32)
    try:
        assert call(renderer.h, _params(rt, W, H, spp), out) == "RT_ERR_UNSUPPORTED"
    finally:
        renderer.set_precision(rt.RT_PREC_F64)
    fresh = rt.Renderer(0)
    try:
        assert call(fresh.h, _params(rt, W, H, spp), out) == "RT_ERR_NO_SCENE"
    finally:
        fresh.close()
    # the context still renders, features and frames, and rt_render's bits did not move
    a, n, d = renderer.render_features(cam, _params(rt, W, H, spp))
    assert np.array_equal(a, bufs[0]) and np.array_equal(n, bufs[1]) and np.array_equal(d, bufs[2])
    assert np.array_equal(renderer.render(cam, p_render), before)
