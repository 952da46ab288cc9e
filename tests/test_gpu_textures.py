"""The kernels' textures against the independent reference's fixture (tests/golden/texture_expected.npz).

rt_trace_rays returns the albedo at a point the caller chooses, so csrc/trace_shade.hpp's tex_value
is compared with tests/texture_reference.py one point at a time, without going through
oracle/oracle.c: the fixture was computed with exact rationals and mpmath
(tests/golden/make_texture_fixture.py; tests/test_texture_reference.py regenerates it on the CPU and
holds the oracle to it), and this file only reads it. The points and worlds are those of
tests/texture_points.py; the bars are the CPU test's: checker, image and the hand-derived records
equal, the noise within 2^-53 (4096 + 4 |scale z|) of the reference (derived in
tests/texture_reference.py; the f64 kernels are built without contraction, which that derivation
would cover too).

Each world runs once per compiled feature set that can hold it, selected with
RT_OPT_EXTRA_FEATURES as tests/test_gpu_f32_exact.py does: the spheres and rect / instance sets
compile tex_value's checker-only shortcut, the final and all sets its switch. Each world is traced
through host pointers under every set and through device pointers under its own.

A plane world's rays land exactly: the hit must be t = 1 at the point itself. A carrier world's
points are rounded: the hit must first reproduce the fixture's material and p bit for bit (the
oracle's, which tests/test_gpu_trace_rays_oracle.py measured equal on 14 worlds); if it does not, the
test fails on that precondition and does not judge the albedo.

The `unpinned` classes (a coordinate of 2^25 or more, where the reference itself overflows; |10 p_i|
or |scale z| beyond the sine's domain of 2^20 pi / 2) are compared with the oracle only, bit for
bit: there the values are deterministic, and nothing else is claimed.
"""
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import texture_points as tp

pytestmark = pytest.mark.gpu

SPHERES, RECTINST, MEDIA, FINAL, ALL = 0, 35, 103, 287, 4095
# world kind -> (RT_OPT_EXTRA_FEATURES, the variant it must select): the first is the world's own
VARIANTS = {
    "checker": [(0, RECTINST), (4, MEDIA), (8, FINAL), (ALL, ALL)],
    "noise": [(0, FINAL), (ALL, ALL)],
    "image": [(0, ALL)],                      # an image on a rect stores its uv: the all-features set only
    "plain": [(0, SPHERES), (1, RECTINST), (5, MEDIA), (8, FINAL), (ALL, ALL)],
    "spheres": [(0, FINAL), (ALL, ALL)],
    "nested": [(0, ALL)],
}
PLANE_CASES = [(tex, axis, extra, variant) for tex in tp.PLANE_TEXTURES for axis in range(3)
               for extra, variant in VARIANTS[tex if tex in ("checker", "image") else "noise"]]
CARRIER_CASES = [(name, extra, variant) for name in tp.CARRIER_WORLDS for extra, variant in VARIANTS[name]]

_fixture, _twins = {}, {}


def fixture():
    if not _fixture:
        with np.load(tp.FIXTURE) as f:
            _fixture.update({k: f[k] for k in f.files})
    return _fixture


def twin(rt, key, build):
    if key not in _twins:
        tw = ob.TwinWorld(rt, tp.SCENE_SEED)
        _twins[key] = (tw, build(tw))
    return _twins[key]


def trace(rt, renderer, world, rays, extra, variant, device):
    """The records and albedo of `rays` under the feature set `extra` selects; through device pointers too
    if asked, which must give the same bytes."""
    extra0 = renderer.get_option(rt.RT_OPT_EXTRA_FEATURES)
    try:
        renderer.set_option(rt.RT_OPT_EXTRA_FEATURES, extra)
        renderer.upload(world)
        hits, alb = renderer.trace_rays(rays, seed=tp.QUERY_SEED, bounce=0, albedo=True)
        st = renderer.query_stats()
        assert st.invalid == 0 and st.rays == len(rays) and st.variant_features == variant, (st.invalid, st.variant_features)
        if device:
            import torch
            dev = torch.device("cuda", 0)
            d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).to(dev)
            d_hits = torch.full((len(rays) * 80,), 0xAB, dtype=torch.uint8, device=dev)
            d_alb = torch.full((len(rays), 3), 7.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            stream = torch.cuda.Stream(dev)
            renderer.trace_rays_device(d_rays.data_ptr(), len(rays), rt.RT_QUERY_CLOSEST, hits_ptr=d_hits.data_ptr(),
                                       albedo_ptr=d_alb.data_ptr(), seed=tp.QUERY_SEED, stream=stream.cuda_stream)
            assert renderer.query_stats().variant_features == variant      # waits for the kernel
            stream.synchronize()
            assert d_hits.cpu().numpy().tobytes() == hits.tobytes(), "device pointers: other records"
            assert d_alb.cpu().numpy().tobytes() == alb.tobytes(), "device pointers: other albedo"
    finally:
        renderer.set_option(rt.RT_OPT_EXTRA_FEATURES, extra0)
    return hits, alb


def same_bits(a, b):
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("tex,axis,extra,variant", PLANE_CASES)
def test_plane_points_match_the_reference(rt, renderer, tex, axis, extra, variant):
    f, name = fixture(), f"{tex}_{axis}"
    s = tp.plane_set(tex, axis)
    assert np.array_equal(tp.ray_sha(s.rays), f[f"{name}.sha"]), "the rays are not the ones the fixture was made for"
    tw, _ = twin(rt, name, lambda t: tp.plane_world(t, tex, axis))
    hits, alb = trace(rt, renderer, tw.product, s.rays, extra, variant, device=extra == 0)
    # the ray lands on the point itself: t = 1, nothing rounds
    assert (hits["t"] == 1.0).all() and np.array_equal(hits["p"], s.pts), name
    assert np.array_equal(hits["mat"], np.array([tp.K.index(k) for k in s.pts[:, tp.PLANE_AXIS[axis]]]) % 2)
    scale_z = tp.NOISE_SCALES.get(tex, 0.0) * s.pts[:, 2]
    share = tp.judge(alb, f, name, scale_z, s.classes, s.cls, f"{name} variant {variant}")
    assert share <= 0.25
    # beyond 2^25 and beyond the sine's domain: the oracle's bits, and nothing else is claimed
    if not s.pinned.all():
        ref = tw.oracle.hit(s.rays[~s.pinned], tp.QUERY_SEED, 0)
        assert (ref["hit"] != 0).all() and same_bits(alb[~s.pinned], ref["albedo"]).all(), name
        print(f"{name}: {int((~s.pinned).sum())} unpinned points equal the oracle bit for bit")


@pytest.mark.parametrize("name,extra,variant", CARRIER_CASES)
def test_carriers_match_the_reference(rt, renderer, name, extra, variant):
    f = fixture()
    build, make_set = tp.CARRIER_WORLDS[name]
    rays, _ = make_set()
    assert np.array_equal(tp.ray_sha(rays), f[f"{name}.sha"]), "the rays are not the ones the fixture was made for"
    tw, carriers = twin(rt, name, build)
    hits, alb = trace(rt, renderer, tw.product, rays, extra, variant, device=extra == 0)
    # the precondition: the fixture's material and p, bit for bit
    code, mat = f[f"{name}.code"], f[f"{name}.mat"].astype(np.int32)
    hit = np.isfinite(hits["t"])
    assert np.array_equal(hit, code != tp.CODE_MISS), f"{name}: precondition: hit / miss differs from the fixture's"
    assert np.array_equal(hits["mat"], mat - 1), f"{name}: precondition: a ray ends on another material"
    assert hits["p"][hit].tobytes() == f[f"{name}.p"].tobytes(), \
        f"{name}: precondition: p differs from the fixture's on hits {np.flatnonzero((hits['p'][hit] != f[f'{name}.p']).any(1))[:10]}"
    names = sorted({c.name for c in carriers.values()} | {"miss"})
    cls = np.array([names.index(carriers[int(m)].name if h else "miss") for m, h in zip(mat, hit)])
    share = tp.judge(alb, f, name, tp.NOISE_CARRIER_SCALE * hits["p"][:, 2], names, cls, f"{name} variant {variant}")
    assert share <= 0.25 and (alb[~hit] == 0).all()
    assert (code != tp.CODE_UNPINNED).all()       # no sphere- or instance-borne point was left out


def test_device_numerics_bit_equal_host_at_hard_points(rt, renderer):
    """renderer.device_eval against the host's rt_numerics.h (ob.evaluate) on the hard-point sets of
    tests/test_texture_reference.py, which holds the host to mpmath there: the doubles within 3 ulp of
    k pi / 2 over the sine's whole domain and past its end, atan2 on the axes and at signed zeros, acos
    at +-1, log next to 1. The rules of test_device_numerics_bit_equal_host: the same bits, NaN for NaN."""
    trig = np.concatenate([tp.hard_trig_points(), tp.beyond_trig_points(), [2.0 ** 60, 1e300, -1.7e308]])
    y, x = tp.hard_atan2_points()
    cases = {0: (trig,), 1: (trig,), 12: (trig,), 3: (y, x), 4: (tp.hard_acos_points(),), 2: (tp.hard_log_points(),)}
    for fn, args in cases.items():
        host = ob.evaluate(fn, *args)
        dev = renderer.device_eval(fn, *args)
        same = same_bits(host, dev)
        assert same.all(), f"fn {fn}: {int((~same).sum())} of {same.size} differ, e.g. at {[a[~same][:3] for a in args]}"
