"""rt_trace_rays on the device: closest-hit and occlusion queries for caller rays (include/rt/rt_abi.h).

Frames are 37x21 (777 rays: the spheres variant's 768-thread workgroup plus nine, three 256-thread
workgroups plus a ragged tail) and 9x5. The worlds are tests/test_gpu_features.py's WORLDS, one per
kernel variant, under its cameras at aperture 0.1.

Against the feature pass, bit for bit: the rays of rt_camera_rays for samples 0, 1, 2, traced as
CLOSEST queries and summed in numpy from 0.0 in sample order, times 1/3, are rt_render_features'
albedo, normal and depth at spp 3 in one chunk (a miss contributes the background to the albedo there
and zeros here: the test puts the background in); at spp 1 per record. That pins the lens and time
draws of rt_camera_rays (the spheres world moves) and the medium's key. Against the oracle: sample
0's albedo is the LightTwin's render at max_depth 1. Against numpy: tests/query_reference.py's
closest hit over the SIMPLE worlds on its 1,000 caller rays with per-ray intervals, 1e-9 absolute
plus relative, the hit / miss classification equal on every ray (tests/test_camera_rays.py asserts
the set's margins, so no ray is excluded). Ids against the flattened tables. ANY against CLOSEST.
Then what must not change the bits, the invalid rays, and the error codes.

rt_hit.mat on a medium's hit. The record carries the medium's phase function: prims[prim].mat when
the medium is the top-level primitive; when it sits under an instance, prim is the instance (whose
record has no material) and the medium is its child, so the test reads the medium's record there.
"""
import ctypes

import numpy as np
import pytest

from tests import features_reference as fr
from tests import query_reference as qr
from tests import test_gpu_features as tf
from tests.test_gpu_parity import assert_parity
from tests.test_primary_candidates import PRIM

pytestmark = pytest.mark.gpu

BG = tf.BG
FRAMES = [(37, 21), (9, 5)]
SEED = 1
NODE = np.dtype([("lo0", "<f4", (3,)), ("hi0", "<f4", (3,)), ("lo1", "<f4", (3,)), ("hi1", "<f4", (3,)),
                 ("child", "<i4", (2,)), ("pad", "<i4", (2,))])
INSTANCE = np.dtype([("n_ops", "<i4"), ("child_kind", "<i4"), ("child", "<i4"), ("pad", "<i4"), ("op_kind", "<i4", (4,)),
                     ("op", "<f8", (4, 3))])
K_INSTANCE, K_MEDIUM = 6, 7


def _setup(rt, renderer, monkeypatch, name, W, H, accel=None):
    tw, view = tf._world(rt, monkeypatch, name)
    cam = tf._camera(rt, view, W, H)
    renderer.upload(tw.product, rt.RT_ACCEL_SAH if accel is None else accel)
    return tw, cam


def _same(a, b):
    """Two record arrays equal byte for byte (NaNs included)."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _depth(rays, hits):
    e = hits["p"] - rays["o"]
    d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
    return np.where(np.isfinite(hits["t"]), d, 0.0)


def _features(rays, hits, alb):
    """(n, 7): the sample's contribution to rt_render_features' seven channels."""
    miss = ~np.isfinite(hits["t"])
    a = np.where(miss[:, None], np.array(BG), alb)
    return np.concatenate([a, hits["n"], _depth(rays, hits)[:, None]], axis=-1)


# ---- against the feature pass, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("name", list(tf.WORLDS))
def test_camera_ray_queries_are_the_feature_pass(rt, renderer, monkeypatch, name, W, H):
    tw, cam = _setup(rt, renderer, monkeypatch, name, W, H)
    total = np.zeros((W * H, 7))
    first = None
    for s in range(3):
        rays = rt.camera_rays(cam, W, H, SEED, s)
        hits, alb = renderer.trace_rays(rays, seed=SEED, albedo=True)
        st = renderer.query_stats()
        assert st.variant_features == tf.WORLDS[name][0] and st.rays == W * H and st.invalid == 0 and st.kernel_ms > 0
        assert st.mode == rt.RT_QUERY_CLOSEST and st.batches == 1
        assert np.array_equal(hits["key_pixel"], np.arange(W * H)) and (hits["key_sample"] == s).all()
        miss = ~np.isfinite(hits["t"])
        assert (hits["flags"] & rt.RT_HIT_INVALID == 0).all() and not np.isnan(hits["t"]).any()
        assert (alb[miss] == 0).all() and (hits["p"][miss] == 0).all() and (hits["n"][miss] == 0).all()
        f = _features(rays, hits, alb)
        first = f if first is None else first
        total = total + f
    mean = total * (1.0 / 3.0)
    a, n, d = renderer.render_features(cam, tf._params(rt, W, H, 3, 3))
    want = np.concatenate([a, n, d[..., None]], axis=-1).reshape(W * H, 7)
    assert np.array_equal(mean, want)
    a, n, d = renderer.render_features(cam, tf._params(rt, W, H, 1))
    assert np.array_equal(first, np.concatenate([a, n, d[..., None]], axis=-1).reshape(W * H, 7))
    if name == "spheres":   # the world moves: the time draw matters
        assert renderer.query_stats().variant_features == 0


# ---- against the oracle -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tf.WORLDS))
def test_albedo_matches_the_oracle_light_twin(rt, renderer, monkeypatch, name):
    W, H = FRAMES[0]
    tw, cam = _setup(rt, renderer, monkeypatch, name, W, H)
    rays = rt.camera_rays(cam, W, H, SEED, 0)
    hits, alb = renderer.trace_rays(rays, seed=SEED, albedo=True)
    miss = ~np.isfinite(hits["t"])
    assert 0 < int(miss.sum()) < W * H, int(miss.sum())
    got = np.where(miss[:, None], np.array(BG), alb).reshape(H, W, 3)
    ref = tw.oracle.render(fr.cam24(cam), BG, W, H, 1, max_depth=1)
    assert_parity(got, ref, f"query albedo, {name} {W}x{H}")
    # albedo alone is a valid output set, and the same values
    n = W * H
    only = np.zeros((n, 3))
    p = rt.QueryParams(n=n, mode=rt.RT_QUERY_CLOSEST, seed=SEED)
    out = rt.QueryOut(None, only.ctypes.data, None)
    assert rt.load_library().rt_trace_rays(renderer.h, ctypes.byref(p), rays.ctypes.data, ctypes.byref(out)) == rt.RT_OK
    assert np.array_equal(only, alb)


# ---- against numpy on caller rays --------------------------------------------------------------------
_caller = {}


def _caller_set(rt, name):
    if name not in _caller:
        prims = tf.SIMPLE[name][0]
        o, d, t_min, t_max, cls = qr.caller_rays(prims)
        _caller[name] = (qr.as_rays(rt.RAY, o, d, t_min, t_max), qr.closest_hit(prims, o, d, t_min, t_max), cls)
    return _caller[name]


@pytest.mark.parametrize("name", list(tf.SIMPLE))
def test_caller_rays_match_the_numpy_closest_hit(rt, renderer, name):
    prims, mats, variant = tf.SIMPLE[name]
    rays, ref, cls = _caller_set(rt, name)
    renderer.upload(fr.build_simple(rt, prims, mats))
    hits = renderer.trace_rays(rays)
    st = renderer.query_stats()
    assert st.variant_features == variant and st.invalid == 0 and st.rays == qr.N_RAYS
    hit = np.isfinite(hits["t"])
    assert np.array_equal(hit, np.isfinite(ref["t"])), "hit / miss classification"
    assert not np.isnan(hits["t"]).any() and np.isposinf(hits["t"][~hit]).all()
    for f in ("t", "p", "n"):
        got, want = hits[f][hit], ref[f][hit]
        err = float(np.max(np.abs(got - want) / (1e-9 + 1e-9 * np.abs(want))))
        print(f"{name} {f}: max |got - ref| / (1e-9 + 1e-9 |ref|) = {err:.3e}")
        assert err <= 1.0, f
    assert np.array_equal((hits["flags"] & rt.RT_HIT_FRONT) != 0, ref["front"])
    assert (hits["flags"] & ~rt.RT_HIT_FRONT == 0).all()
    assert np.array_equal(hits["mat"], ref["index"])    # build_simple: primitive i carries material i
    assert (hits["prim"] == hits["inner"]).all() and np.array_equal(hits["prim"] >= 0, hit)
    assert np.array_equal(hits["key_pixel"], rays["key_pixel"])


# ---- ids ------------------------------------------------------------------------------------------------
def _tables(soa):
    def table(ptr, n, dt):
        return np.frombuffer(ctypes.string_at(ptr, n * dt.itemsize), dtype=dt).copy() if n else np.zeros(0, dt)
    return (table(soa.prims, soa.n_prims, PRIM), table(soa.prim_refs, soa.n_prim_refs, np.dtype("<i4")),
            table(soa.nodes, soa.n_nodes, NODE), table(soa.instances, soa.n_instances, INSTANCE))


def _top_level(soa, refs, nodes):
    """The prims a walk from tlas_root reaches: the top-level records."""
    top, stack = set(), [soa.tlas_root]
    while stack:
        ref = stack.pop()
        if ref == -2 ** 31:
            continue
        if ref >= 0:
            stack += [int(c) for c in nodes["child"][ref]]
        else:
            code = ~ref
            top.update(int(refs[j]) for j in range(code >> 5, (code >> 5) + (code & 31)))
    return top


@pytest.mark.parametrize("name", ["final", "all"])
def test_ids_name_the_flattened_records(rt, renderer, monkeypatch, name):
    W, H = FRAMES[0]
    tw, cam = _setup(rt, renderer, monkeypatch, name, W, H)
    soa = tw.product.flatten()
    prims, refs, nodes, instances = _tables(soa)
    top = _top_level(soa, refs, nodes)
    hits = np.concatenate([renderer.trace_rays(rt.camera_rays(cam, W, H, SEED, s), seed=SEED) for s in range(2)])
    hit = np.isfinite(hits["t"])
    assert hit.any() and (~hit).any()
    for f in ("prim", "inner", "mat"):
        assert (hits[f][~hit] == -1).all(), f
    h = hits[hit]
    assert ((h["prim"] >= 0) & (h["prim"] < soa.n_prims) & (h["inner"] >= 0) & (h["inner"] < soa.n_prims)).all()
    assert set(h["prim"].tolist()) <= top
    assert (prims["kind"][h["inner"]] <= 5).all()        # a sphere (moving or not), a rect or a box
    medium = (h["flags"] & rt.RT_HIT_MEDIUM) != 0
    kind = prims["kind"][h["prim"]]
    # the medium whose record it is: the top-level primitive, or the child of the top-level instance
    under = medium & (kind == K_INSTANCE)
    inst_of = np.where(kind == K_INSTANCE, prims["a"][h["prim"]], 0)      # the top-level instance's index (0 elsewhere)
    mprim = np.where(under, instances["child"][inst_of], h["prim"])
    assert (prims["kind"][mprim[medium]] == K_MEDIUM).all()
    assert np.array_equal(h["mat"][medium], prims["mat"][mprim[medium]])
    assert np.array_equal(h["mat"][~medium], prims["mat"][h["inner"][~medium]])
    assert ((kind == K_MEDIUM) <= medium).all()
    simple = kind <= 5
    assert np.array_equal(h["inner"][simple], h["prim"][simple])
    inst = (kind == K_INSTANCE) & ~medium
    assert (h["inner"][inst] != h["prim"][inst]).all()
    # the worlds show what they were built for: simple, instanced and medium hits; a BLAS under an instance
    assert simple.any() and inst.any() and medium.any()
    blas = inst & (instances["child_kind"][inst_of] == 1)
    assert blas.any() and len(set(h["inner"][blas].tolist())) > 1
    if name == "all":
        assert under.any() and (prims["kind"][h["inner"][inst]] == 5).any()   # a medium and a box under instances


# ---- ANY is "CLOSEST reports a hit" -------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tf.WORLDS))
def test_any_equals_closest_on_camera_rays(rt, renderer, monkeypatch, name):
    W, H = FRAMES[0]
    tw, cam = _setup(rt, renderer, monkeypatch, name, W, H)
    rays = rt.camera_rays(cam, W, H, SEED, 0)
    hit = np.isfinite(renderer.trace_rays(rays, seed=SEED)["t"])
    occ = renderer.trace_rays(rays, mode=rt.RT_QUERY_ANY, seed=SEED)
    st = renderer.query_stats()
    assert st.mode == rt.RT_QUERY_ANY and st.invalid == 0 and st.kernel_ms > 0
    assert occ.dtype == bool and np.array_equal(occ, hit)
    assert occ.any() and (~occ).any()


@pytest.mark.parametrize("name", list(tf.SIMPLE))
def test_any_equals_closest_on_finite_segments(rt, renderer, name):
    prims, mats, variant = tf.SIMPLE[name]
    rays = _caller_set(rt, name)[0].copy()
    rays["t_max"] = np.where(np.isinf(rays["t_max"]), 3.0, rays["t_max"])
    rays = rays[rays["t_min"] <= rays["t_max"]]
    assert len(rays) > 900 and np.isfinite(rays["t_max"]).all()
    renderer.upload(fr.build_simple(rt, prims, mats))
    hit = np.isfinite(renderer.trace_rays(rays)["t"])
    occ = renderer.trace_rays(rays, mode=rt.RT_QUERY_ANY)
    assert np.array_equal(occ, hit) and occ.any() and (~occ).any()


# ---- what must not change the bits ----------------------------------------------------------------------
def _both(r, rays, rt):
    hits, alb = r.trace_rays(rays, seed=SEED, albedo=True)
    return hits, alb, r.trace_rays(rays, mode=rt.RT_QUERY_ANY, seed=SEED)


def test_bits_do_not_depend_on_the_acceleration_structure(rt, renderer, monkeypatch):
    W, H = FRAMES[0]
    tw, view = tf._world(rt, monkeypatch, "all")
    cam = tf._camera(rt, view, W, H)
    rays = rt.camera_rays(cam, W, H, SEED, 0)
    got = []
    for accel in (rt.RT_ACCEL_SAH, rt.RT_ACCEL_LINEAR, rt.RT_ACCEL_MEDIAN):
        renderer.upload(tw.product, accel)
        got.append(_both(renderer, rays, rt))
    for other in got[1:]:
        hits, alb, occ = other
        for f in ("t", "p", "n", "prim", "mat", "flags", "key_pixel", "key_sample"):
            assert hits[f].tobytes() == got[0][0][f].tobytes(), f
        # inner too, but for a medium bounded by a BVH, where it is some primitive of that BVH (rt_abi.h)
        solid = (hits["flags"] & rt.RT_HIT_MEDIUM) == 0
        assert np.array_equal(hits["inner"][solid], got[0][0]["inner"][solid])
        assert np.array_equal(alb, got[0][1]) and np.array_equal(occ, got[0][2])
    assert np.isfinite(got[0][0]["t"]).any()


def test_bits_do_not_depend_on_the_kernel_variant(rt, renderer, monkeypatch):
    W, H = FRAMES[0]
    tw, cam = _setup(rt, renderer, monkeypatch, "spheres", W, H)
    rays = rt.camera_rays(cam, W, H, SEED, 0)
    want = _both(renderer, rays, rt)
    assert renderer.query_stats().variant_features == 0
    r = rt.Renderer(0)
    try:
        r.set_option(rt.RT_OPT_EXTRA_FEATURES, 4095)
        r.upload(tw.product)
        got = _both(r, rays, rt)
        assert r.query_stats().variant_features == 4095
    finally:
        r.close()
    assert _same(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_shuffles_prefixes_and_an_empty_call(rt, renderer, monkeypatch):
    W, H = FRAMES[0]
    tw, cam = _setup(rt, renderer, monkeypatch, "final", W, H)
    rays = rt.camera_rays(cam, W, H, SEED, 0)
    hits, alb, occ = _both(renderer, rays, rt)
    perm = np.random.default_rng(5).permutation(W * H)
    h2, a2, o2 = _both(renderer, rays[perm], rt)
    assert _same(h2, hits[perm]) and np.array_equal(a2, alb[perm]) and np.array_equal(o2, occ[perm])
    assert np.array_equal(h2["key_pixel"], perm)          # the echoed keys say where each record came from
    tiled = rt.camera_rays(cam, W, H, SEED, 0, tiled=True)
    ht = renderer.trace_rays(tiled, seed=SEED)
    assert _same(ht, hits[ht["key_pixel"]]) and sorted(ht["key_pixel"].tolist()) == list(range(W * H))
    for n in (1, 63, 64, 65):
        hn, an, on = _both(renderer, rays[:n], rt)
        assert _same(hn, hits[:n]) and np.array_equal(an, alb[:n]) and np.array_equal(on, occ[:n]), n
        assert renderer.query_stats().rays == n
    lib = rt.load_library()
    p = rt.QueryParams(n=0, mode=rt.RT_QUERY_CLOSEST, seed=SEED)
    untouched = hits.copy()
    out = rt.QueryOut(untouched.ctypes.data, None, None)
    assert lib.rt_trace_rays(renderer.h, ctypes.byref(p), rays.ctypes.data, ctypes.byref(out)) == rt.RT_OK
    assert _same(untouched, hits) and renderer.query_stats().rays == 0


def test_buffer_batches_keep_the_bits(rt, renderer, monkeypatch):
    """151x115 = 17,365 rays with hits and albedo: 184 device bytes per ray, so a bound of 1 MiB (the
    option's minimum) holds 5,698 rays and the call takes 4 batches; the default bound takes one."""
    W, H = 151, 115
    tw, cam = _setup(rt, renderer, monkeypatch, "spheres", W, H)
    rays = rt.camera_rays(cam, W, H, SEED, 0)
    want = _both(renderer, rays, rt)
    assert renderer.query_stats().batches == 1
    r = rt.Renderer(0)
    try:
        r.set_option(rt.RT_OPT_TRACE_BUF_BYTES, 1 << 20)
        r.upload(tw.product)
        hits, alb = r.trace_rays(rays, seed=SEED, albedo=True)
        st = r.query_stats()
        assert st.batches == 4 and st.rays == W * H and st.kernel_ms > 0
        occ = r.trace_rays(rays, mode=rt.RT_QUERY_ANY, seed=SEED)
        assert r.query_stats().batches == 2     # 81 bytes per ray
    finally:
        r.close()
    assert _same(hits, want[0]) and np.array_equal(alb, want[1]) and np.array_equal(occ, want[2])


def _device_query(rt, renderer, rays, mode, origin_bound, albedo=True):
    """The query through device pointers on a torch stream; (hits, albedo) or occluded, and the stats."""
    import torch
    n = len(rays)
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
    d_hits = torch.full((n * 80,), 0xAB, dtype=torch.uint8, device=dev)
    d_alb = torch.full((n, 3), 7.0, dtype=torch.float64, device=dev)
    d_occ = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(dev)
    if mode == rt.RT_QUERY_ANY:
        renderer.trace_rays_device(d_rays.data_ptr(), n, mode, occluded_ptr=d_occ.data_ptr(), seed=SEED,
                                   origin_bound=origin_bound, stream=stream.cuda_stream)
    else:
        renderer.trace_rays_device(d_rays.data_ptr(), n, mode, hits_ptr=d_hits.data_ptr(),
                                   albedo_ptr=d_alb.data_ptr() if albedo else 0, seed=SEED, origin_bound=origin_bound,
                                   stream=stream.cuda_stream)
    st = renderer.query_stats()     # waits for the kernel
    stream.synchronize()
    assert st.kernel_ms > 0 and st.invalid == -1 and st.rays == n
    if mode == rt.RT_QUERY_ANY:
        return d_occ.cpu().numpy().astype(bool), st
    return (d_hits.cpu().numpy().view(rt.HIT), d_alb.cpu().numpy()), st


def test_device_pointers_and_slab_precision_keep_the_bits(rt, renderer, monkeypatch):
    W, H = FRAMES[0]
    tw, cam = _setup(rt, renderer, monkeypatch, "final", W, H)
    rays = rt.camera_rays(cam, W, H, SEED, 0)
    hits, alb, occ = _both(renderer, rays, rt)
    host_slab32 = renderer.query_stats().slab32
    bound = float(np.abs(rays["o"]).max())
    (h32, a32), st32 = _device_query(rt, renderer, rays, rt.RT_QUERY_CLOSEST, bound)
    (h64, a64), st64 = _device_query(rt, renderer, rays, rt.RT_QUERY_CLOSEST, 0.0)
    assert st32.slab32 == 1 and host_slab32 == 1 and st64.slab32 == 0      # f32 slabs against f64 slabs
    assert _same(h32, hits) and np.array_equal(a32, alb)
    assert _same(h64, hits) and np.array_equal(a64, alb)
    o32, _ = _device_query(rt, renderer, rays, rt.RT_QUERY_ANY, bound)
    o64, st = _device_query(rt, renderer, rays, rt.RT_QUERY_ANY, float("inf"))
    assert st.slab32 == 0 and np.array_equal(o32, occ) and np.array_equal(o64, occ)
    (hn, _), _ = _device_query(rt, renderer, rays, rt.RT_QUERY_CLOSEST, bound, albedo=False)
    assert _same(hn, hits)


def test_a_query_leaves_rt_render_alone(rt, renderer, monkeypatch):
    W, H = 24, 16
    tw, cam = _setup(rt, renderer, monkeypatch, "spheres", W, H)
    p = rt.Renderer.params(W, H, 4, 50, BG, SEED, out_format=rt.RT_OUT_F64)
    before = renderer.render(cam, p).copy()
    rays = rt.camera_rays(cam, W, H, SEED, 0)
    hits = renderer.trace_rays(rays, seed=SEED)
    assert np.array_equal(renderer.render(cam, p), before)
    assert _same(renderer.trace_rays(rays, seed=SEED), hits)     # and a render leaves the query alone


# ---- invalid rays ---------------------------------------------------------------------------------------
def test_invalid_rays_end_as_flags(rt, renderer, monkeypatch):
    W, H = FRAMES[0]
    tw, cam = _setup(rt, renderer, monkeypatch, "spheres", W, H)      # (a moving sphere: ray times are checked)
    clean = rt.camera_rays(cam, W, H, SEED, 0)
    hits, alb, occ = _both(renderer, clean, rt)
    rays = clean.copy()
    rays["o"][3, 0] = np.nan                       # a NaN origin
    rays["d"][100] = 0.0                           # a zero direction
    rays["t_min"][200], rays["t_max"][200] = 5.0, 1.0
    rays["t_max"][300] = np.nan
    rays["time"][400] = 2.0                        # outside the scene's [0, 1]
    bad = np.zeros(W * H, dtype=bool)
    bad[[3, 100, 200, 300, 400]] = True

    def check(h, a, o, bad):
        assert np.array_equal((h["flags"] & rt.RT_HIT_INVALID) != 0, bad)
        assert np.isnan(h["t"][bad]).all() and (h["flags"][bad] == rt.RT_HIT_INVALID).all()
        for f in ("p", "n"):
            assert (h[f][bad] == 0).all()
        for f in ("prim", "inner", "mat"):
            assert (h[f][bad] == -1).all()
        assert np.array_equal(h["key_pixel"], clean["key_pixel"])
        assert (a[bad] == 0).all() and not o[bad].any()
        assert _same(h[~bad], hits[~bad]) and np.array_equal(a[~bad], alb[~bad]) and np.array_equal(o[~bad], occ[~bad])

    h, a = renderer.trace_rays(rays, seed=SEED, albedo=True)
    assert renderer.query_stats().invalid == 5
    o = renderer.trace_rays(rays, mode=rt.RT_QUERY_ANY, seed=SEED)
    assert renderer.query_stats().invalid == 5
    check(h, a, o, bad)
    # the sixth defect: an origin beyond the bound a device-pointer call states
    bound = float(np.abs(clean["o"]).max())
    rays["o"][500] = (bound * 1.5, 0.0, 0.0)
    bad[500] = True
    (h, a), st = _device_query(rt, renderer, rays, rt.RT_QUERY_CLOSEST, bound)
    o, _ = _device_query(rt, renderer, rays, rt.RT_QUERY_ANY, bound)
    check(h, a, o, bad)
    # the same ray under a host-pointer call, which plans with the rays' own bound: walked, not flagged
    h = renderer.trace_rays(rays, seed=SEED)
    assert renderer.query_stats().invalid == 5 and h["flags"][500] & rt.RT_HIT_INVALID == 0
    # an infinite t_min = t_max interval, an inverted infinite one, +-inf ends: decided, never walked for long
    edge = clean[:4].copy()
    edge["t_min"], edge["t_max"] = [-np.inf, np.inf, np.inf, 0.0], [np.inf, np.inf, -np.inf, 0.0]
    h = renderer.trace_rays(edge, seed=SEED)
    assert (h["flags"] & rt.RT_HIT_INVALID != 0).tolist() == [False, False, True, False]
    assert np.isposinf(h["t"][[1, 3]]).all()


# ---- error codes ----------------------------------------------------------------------------------------
def test_error_codes(rt, renderer, monkeypatch):
    W, H = FRAMES[1]
    tw, cam = _setup(rt, renderer, monkeypatch, "spheres", W, H)
    lib = rt.load_library()
    rays = rt.camera_rays(cam, W, H, SEED, 0)
    n = W * H
    hits, alb, occ = np.zeros(n, dtype=rt.HIT), np.zeros((n, 3)), np.zeros(n, dtype=np.uint8)
    H_, A_, O_ = hits.ctypes.data, alb.ctypes.data, occ.ctypes.data

    def call(h, p, r, o):
        return rt.ERRORS.get(lib.rt_trace_rays(h, ctypes.byref(p) if p is not None else None, r,
                                               ctypes.byref(o) if o is not None else None), "RT_OK")

    P = lambda **kw: rt.QueryParams(**{**dict(n=n, mode=rt.RT_QUERY_CLOSEST, seed=SEED), **kw})
    closest, anyq = rt.QueryOut(H_, A_, None), rt.QueryOut(None, None, O_)
    assert call(renderer.h, P(), rays.ctypes.data, closest) == "RT_OK"
    assert call(renderer.h, P(mode=rt.RT_QUERY_ANY), rays.ctypes.data, anyq) == "RT_OK"
    assert call(None, P(), rays.ctypes.data, closest) == "RT_ERR_INVALID"
    assert call(renderer.h, None, rays.ctypes.data, closest) == "RT_ERR_INVALID"
    assert call(renderer.h, P(), None, closest) == "RT_ERR_INVALID"
    assert call(renderer.h, P(), rays.ctypes.data, None) == "RT_ERR_INVALID"
    assert lib.rt_last_error()
    assert call(renderer.h, P(), rays.ctypes.data, rt.QueryOut(None, None, None)) == "RT_ERR_INVALID"
    assert call(renderer.h, P(), rays.ctypes.data, rt.QueryOut(H_, None, O_)) == "RT_ERR_INVALID"
    assert call(renderer.h, P(mode=rt.RT_QUERY_ANY), rays.ctypes.data, rt.QueryOut(None, None, None)) == "RT_ERR_INVALID"
    assert call(renderer.h, P(mode=rt.RT_QUERY_ANY), rays.ctypes.data, rt.QueryOut(H_, None, O_)) == "RT_ERR_INVALID"
    assert call(renderer.h, P(mode=rt.RT_QUERY_ANY), rays.ctypes.data, rt.QueryOut(None, A_, O_)) == "RT_ERR_INVALID"
    assert call(renderer.h, P(mode=2), rays.ctypes.data, closest) == "RT_ERR_INVALID"
    assert call(renderer.h, P(n=-1), rays.ctypes.data, closest) == "RT_ERR_INVALID"
    assert call(renderer.h, P(n=2 ** 31), rays.ctypes.data, closest) == "RT_ERR_INVALID"
    assert call(renderer.h, P(on_device=1), rays.ctypes.data + 8, closest) == "RT_ERR_INVALID"   # misaligned device records
    renderer.set_precision(rt.RT_PREC_F32)
    try:
        assert call(renderer.h, P(), rays.ctypes.data, closest) == "RT_ERR_UNSUPPORTED"
    finally:
        renderer.set_precision(rt.RT_PREC_F64)
    fresh = rt.Renderer(0)
    try:
        assert call(fresh.h, P(), rays.ctypes.data, closest) == "RT_ERR_NO_SCENE"
        assert rt.ERRORS.get(lib.rt_query_last_stats(fresh.h, None)) == "RT_ERR_INVALID"
    finally:
        fresh.close()
    # the context still answers, with the same records
    again = renderer.trace_rays(rays, seed=SEED)
    assert _same(again, hits)
