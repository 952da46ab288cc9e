"""rt_trace_rays held to the oracle's hit records on caller rays (include/rt/rt_abi.h).

tests/test_gpu_trace_rays.py compares a query with the feature pass, which runs the same device
functions (instance_t, medium_t, finish_hit, instance_finish), and with a numpy reference that knows
top-level static spheres and rects only. Here the reference is oracle/oracle.c's restatement of
hit_hittables, asked through orc_world_hit / orc_scene_hit for the caller's own rays: t, p, n, the
front flag, the material and the winner's place in the world's list, for origins on surfaces and
inside spheres, boxes, medium boundaries and instanced clusters, unnormalised directions, ray times
over the whole range and at its two ends, and the seven interval classes (tests/oracle_rays.py, whose
stability rule keeps only rays the 1e-9 bar can judge; tests/test_oracle_hits.py holds the sets and
the two oracle entries to their own checks on the CPU).

Worlds (WORLDS). The five of tests/test_gpu_features.py, one per kernel variant, built through
oracle_binding.TwinWorld, so both sides carry the same materials; `edges`: a negative-radius sphere
inside a glass sphere, a top-level box, a moving sphere whose shutter is (1, 0), a chain of four
translate / rotate_y ops, two overlapping media, a medium under two instances and a medium bounded
by a BVH; and the built-in scenes 0, 1, 2, 4, 5, 6 and 7 at scene seed 1 (3, one sphere, has too few
second hits for a full set; scene 7 carries its image texture) — scene 7 twice, under its own
camera and under one aimed at its 1,000-sphere cluster, the one scene whose nested walk is deep
(SceneFacts.nested_stack_entries 26 against stack_entries 13). rt_hit.mat is compared on every
world: TwinWorld asserts that the two sides' material handles agree, and the built-in scenes'
builders (csrc/scene_model.cpp, oracle.c) register their materials in the same order, main.rs's.
rt_hit.prim against the oracle's `top`: every top-level record belongs to one entry of the world's
list, and an entry is one record except where the lowering dissolves it (DISSOLVED).

Every set is compared whole: 1,000 of 1,000 rays, hit / miss equal on each.

Exact ties. Where two top-level primitives accept the same t (scene 7's ground boxes share their
sides) the record must name the later one of the list under every acceleration structure:
test_scene7_acceleration_structures_give_the_default_records, whose four such rays first showed that
it did not.
"""
import contextlib
from collections import namedtuple

import numpy as np
import pytest

from tests import features_reference as fr
from tests import oracle_binding as ob
from tests import oracle_rays
from tests import test_gpu_features as tf
from tests import test_gpu_nesting as nesting
from tests.test_gpu_parity import assert_parity

pytestmark = pytest.mark.gpu

SEED = 5                     # the keyed draw's seed, on both sides
POOL_W, POOL_H = 64, 40      # the frame whose camera rays seed a set's origins
TIME_RANGE = (0.0, 1.0)      # rt_scene_soa.time_lo / time_hi of every world here


class _Twin(ob.TwinWorld):
    """A TwinWorld that remembers which material handles are phase functions."""

    def __init__(self, rt, scene_seed: int = 1):
        super().__init__(rt, scene_seed)
        self.phase = set()

    def isotropic(self, tex):
        m = super().__getattr__("isotropic")(tex)
        self.phase.add(m)
        return m


@contextlib.contextmanager
def _plain_twins():
    """tests/test_gpu_features.py's builders write to a features_reference.LightTwin and
    tests/test_gpu_nesting.py's to a TwinWorld; inside, both names are _Twin."""
    saved = fr.LightTwin, ob.TwinWorld
    fr.LightTwin = ob.TwinWorld = _Twin
    try:
        yield
    finally:
        fr.LightTwin, ob.TwinWorld = saved


def _edges_world(rt):
    tw = _Twin(rt, 13)
    white = tw.lambertian(tw.solid(0.73, 0.73, 0.73))
    red = tw.lambertian(tw.checker((0.65, 0.05, 0.05), (0.9, 0.9, 0.9)))
    metal = tw.metal((0.8, 0.8, 0.9), 0.1)
    glass = tw.dielectric(1.5)
    haze = tw.isotropic(tw.solid(0.8, 0.8, 0.9))
    moss = tw.isotropic(tw.solid(0.2, 0.7, 0.3))
    tw.push(tw.sphere(white, (0.0, -1000.0, 0.0), 1000.0))
    # a hollow glass ball: the inner sphere's radius is negative (its normal points inward)
    tw.push(tw.sphere(glass, (0.0, 1.0, 0.0), 1.0))
    tw.push(tw.sphere(glass, (0.0, 1.0, 0.0), -0.9))
    tw.push(tw.box((-3.2, 0.0, -0.5), (-2.2, 1.2, 0.6), red))                               # a top-level box
    tw.push(tw.moving_sphere(metal, (2.2, 0.5, 1.5), (2.2, 1.0, 1.5), 1.0, 0.0, 0.5))        # shutter (1, 0)
    # translate(rotate_y(translate(rotate_y(box)))): a chain of four ops
    b = tw.box((0.0, 0.0, 0.0), (0.8, 1.0, 0.8), white)
    tw.push(tw.translate(tw.rotate_y(tw.translate(tw.rotate_y(b, 20.0), (0.3, 0.0, 0.2)), -35.0), (1.5, 0.0, -2.5)))
    # two overlapping media
    tw.push(tw.constant_medium(tw.sphere(white, (-1.5, 0.8, 2.5), 0.8), 1.2, haze))
    tw.push(tw.constant_medium(tw.sphere(white, (-0.7, 0.8, 2.7), 0.8), 0.8, moss))
    # a medium under two instances, its boundary an instanced box
    smoke = tw.constant_medium(tw.translate(tw.rotate_y(tw.box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), white), 15.0),
                                            (-0.5, 0.0, -0.5)), 1.5, haze)
    tw.push(tw.translate(tw.rotate_y(smoke, 40.0), (-2.5, 0.0, -2.5)))
    # a medium bounded by a BVH of two spheres
    tw.push(tw.constant_medium(tw.bvh([tw.sphere(white, (3.0, 0.6, -0.8), 0.6), tw.sphere(white, (3.7, 0.6, -0.8), 0.6)]),
                               1.2, moss))
    return tw, ((7.0, 4.0, 9.0), (0.0, 0.7, 0.0), 40.0)


# name: (kernel variant, what builds it). A twin builder returns (TwinWorld, view); a scene is
# (scene id, phase-function handles in registration order, (look_from, look_at, vfov) or None = its own camera)
WORLDS = {
    "spheres": (0, lambda rt: tf._spheres_world(rt)),
    "rectinst": (35, lambda rt: tf._cornell_world(rt, False)),
    "media": (103, lambda rt: tf._cornell_world(rt, True)),
    "final": (287, lambda rt: tf._final_world(rt)),
    "all": (4095, lambda rt: (nesting._nested_world(rt), ((7.0, 4.0, 9.0), (0.0, 0.7, 0.0), 40.0))),
    "edges": (4095, _edges_world),
    "scene0": (0, (0, (), None)),
    "scene1": (0, (1, (), None)),
    "scene2": (287, (2, (), None)),
    "scene4": (287, (4, (), None)),
    "scene5": (35, (5, (), None)),
    "scene6": (103, (6, (5, 6), None)),
    "scene7": (287, (7, (6, 7), None)),
    # the cluster is Translate(RotateY(BVH of 1,000 spheres in [0, 165]^3, 15), (-100, 270, 395)): its middle
    "scene7_cluster": (287, (7, (6, 7), ((478.0, 278.0, -600.0), (1.0, 352.0, 453.0), 7.0))),
}
MEDIA = ("media", "final", "all", "edges", "scene6", "scene7", "scene7_cluster")
CLUSTER_TOP = 10     # the cluster's place in scene 7's list (oracle.c final_scene: the eleventh push)

# List entries the lowering dissolves into several top-level records (flatten.cpp): a BVH pushed as it is
# (scene 7's 400 boxes) and an instance over a BVH that holds more than plain primitives (the nested
# world's Translate(RotateY(BVH[instanced box, medium, spheres])), whose chain is pushed down to each)
DISSOLVED = {"all": {2}, "scene7": {0}, "scene7_cluster": {0}}

World = namedtuple("World", "name variant product hit_fn cam phase keep")
_worlds, _sets = {}, {}


def world(rt, name):
    """The world's product side (an rt.World to upload), its oracle (hit_fn(rays, bounce) under SEED),
    the camera its sets start from and its phase-function material handles."""
    if name in _worlds:
        return _worlds[name]
    variant, spec = WORLDS[name]
    if callable(spec):
        with _plain_twins():
            tw, view = spec(rt)
        cam = tf._camera(rt, view, POOL_W, POOL_H)
        w = World(name, variant, tw.product, lambda rays, bounce, o=tw.oracle: o.hit(rays, SEED, bounce), cam, frozenset(tw.phase), tw)
    else:
        scene_id, phase, view = spec
        product = rt.World(1).build_scene(scene_id)
        cam = rt.scene_camera(scene_id, POOL_W, POOL_H)[0] if view is None else \
            rt.camera_new(view[0], view[1], (0.0, 1.0, 0.0), view[2], 1.0, 0.1, 10.0, 0.0, 1.0)
        w = World(name, variant, product, lambda rays, bounce, s=scene_id: ob.scene_hit(s, rays, SEED, bounce, scene_seed=1), cam,
                  frozenset(phase), None)
    _worlds[name] = w
    return w


def ray_set(rt, name):
    """The world's caller-ray set (tests/oracle_rays.py); media worlds are held stable at bounce 3 too."""
    if name not in _sets:
        w = world(rt, name)
        _sets[name] = oracle_rays.build_set(w.hit_fn, w.cam, POOL_W, POOL_H, TIME_RANGE, 20261021,
                                            bounces=(0, 3) if name in MEDIA else (0,), rt=rt)
    return _sets[name]


def is_phase(w, mat):
    return np.isin(mat, sorted(w.phase)) if w.phase else np.zeros(mat.shape, dtype=bool)


# ---- the comparison ---------------------------------------------------------------------------------
FIELDS = ("t", "p", "n")


def compare(rt, hits, alb, ref, w, label):
    """A query's records against the oracle's, every ray; returns the largest scaled error per field
    and the index of the worst ray."""
    n = len(ref)
    hit = np.isfinite(hits["t"])
    assert np.array_equal(hit, ref["hit"] != 0), f"{label}: hit / miss differs on rays {np.flatnonzero(hit != (ref['hit'] != 0))[:10]}"
    assert not np.isnan(hits["t"]).any() and np.isposinf(hits["t"][~hit]).all()
    worst = {}
    for f in FIELDS:
        got, want = hits[f][hit], ref[f][hit]
        scaled = np.abs(got - want) / (1e-9 + 1e-9 * np.abs(want))
        err = float(scaled.max()) if scaled.size else 0.0
        worst[f] = (err, int(np.flatnonzero(hit)[np.argmax(scaled.reshape(len(got), -1).max(-1))]) if scaled.size else -1)
        print(f"{label} {f}: max |got - oracle| / (1e-9 + 1e-9 |oracle|) = {err:.3e} over {int(hit.sum())} hits of {n}")
    for f in FIELDS:
        assert worst[f][0] <= 1.0, (label, f, worst[f])
    front = (hits["flags"] & rt.RT_HIT_FRONT) != 0
    assert np.array_equal(front, ref["front_face"] != 0), label
    medium = (hits["flags"] & rt.RT_HIT_MEDIUM) != 0
    assert np.array_equal(medium, hit & is_phase(w, ref["mat"])), label
    assert (hits["flags"] & ~(rt.RT_HIT_FRONT | rt.RT_HIT_MEDIUM) == 0).all()
    assert np.array_equal(hits["mat"], np.where(hit, ref["mat"] - 1, -1)), label     # oracle handles are 1-based
    assert (hits["p"][~hit] == 0).all() and (hits["n"][~hit] == 0).all() and (hits["prim"][~hit] == -1).all()
    if alb is not None:
        assert (alb[~hit] == 0).all()
        assert_parity(alb, ref["albedo"], f"{label} albedo")
        print(f"{label} albedo: max |got - oracle| = {float(np.abs(alb - ref['albedo']).max()):.3e}")
    # the winner's place in the oracle's list and rt_hit.prim name each other: no top-level record
    # answers for two list entries, and a list entry is one record unless the lowering dissolves it
    pairs = set(zip(ref["top"][hit].tolist(), hits["prim"][hit].tolist()))
    assert len(pairs) == len({b for _, b in pairs}), (label, sorted(pairs))
    for top in {a for a, _ in pairs}:
        records = sum(1 for a, _ in pairs if a == top)
        assert records > 1 if top in DISSOLVED.get(w.name, ()) else records == 1, (label, top, sorted(pairs))
    return worst


@pytest.mark.parametrize("name", list(WORLDS))
def test_caller_rays_match_the_oracle(rt, renderer, name):
    w = world(rt, name)
    s = ray_set(rt, name)
    print(f"{name}: redrew {100.0 * s.redrawn:.1f} % of the candidates in {s.rounds} round(s); classes "
          f"{np.bincount(s.cls, minlength=7).tolist()}")
    renderer.upload(w.product)
    hits, alb = renderer.trace_rays(s.rays, seed=SEED, bounce=0, albedo=True)
    st = renderer.query_stats()
    assert st.invalid == 0 and st.variant_features == w.variant and st.rays == oracle_rays.N_RAYS
    assert np.array_equal(hits["key_pixel"], s.rays["key_pixel"]) and np.array_equal(hits["key_sample"], s.rays["key_sample"])
    worst = compare(rt, hits, alb, s.ref[0], w, name)
    f = max(worst, key=lambda k: worst[k][0])
    i = worst[f][1]
    print(f"{name}: largest error {worst[f][0]:.3e} ({f}) on ray {i}: class {int(s.cls[i])}, origin kind {int(s.kind[i])}, "
          f"oracle top {int(s.ref[0]['top'][i])}")
    occ = renderer.trace_rays(s.rays, mode=rt.RT_QUERY_ANY, seed=SEED, bounce=0)
    assert renderer.query_stats().invalid == 0
    assert np.array_equal(occ, s.ref[0]["hit"] != 0)
    if name in MEDIA:
        hits3, alb3 = renderer.trace_rays(s.rays, seed=SEED, bounce=3, albedo=True)
        assert renderer.query_stats().invalid == 0
        compare(rt, hits3, alb3, s.ref[3], w, f"{name} bounce 3")
        assert np.array_equal(renderer.trace_rays(s.rays, mode=rt.RT_QUERY_ANY, seed=SEED, bounce=3), s.ref[3]["hit"] != 0)
        moved = (s.ref[0]["hit"] != s.ref[3]["hit"]) | (s.ref[0]["mat"] != s.ref[3]["mat"])
        print(f"{name}: {int(moved.sum())} rays classified differently at bounce 3")
        assert moved.any(), "the key's bounce is not shown to matter"


# ---- directed thin chords: the medium's second query starts at t1 + 0.0001, in units of t -------------
CHORDS = [(chord, length) for chord in (0.5e-4, 2e-4) for length in (1.0, 2.0)]
DENSE = 1e8    # -log(u) <= 37 for every u a 53-bit draw gives, so the distance drawn is under 3.7e-7: any chord accepts


def _chord_rays(rt, entry_mid_dir):
    """One ray per CHORDS entry from (chord in distance) -> (the chord's midpoint, unit direction);
    the origin lies 3 (sphere) or 200 (box) lengths of travel before the midpoint."""
    rays = np.zeros(len(CHORDS), dtype=rt.RAY)
    for i, (chord, length) in enumerate(CHORDS):
        mid, u, back = entry_mid_dir(chord * length)
        rays["o"][i] = mid - back * u
        rays["d"][i] = length * u
    rays["t_min"], rays["t_max"] = 0.001, np.inf
    rays["key_pixel"] = 1000 + np.arange(len(CHORDS))
    return rays


def _sphere_chord(L):
    # the final world's medium: a sphere at (1.5, 0.7, 1.0), radius 0.7; the ray passes along +z over its top
    c, R = np.array([1.5, 0.7, 1.0]), 0.7
    b = np.sqrt(R * R - 0.25 * L * L)
    return c + np.array([0.0, b, 0.0]), np.array([0.0, 0.0, 1.0]), 3.0


def _box_chord(L):
    # the media world's first medium: translate(rotate_y(box((0, 0, 0), (165, 330, 165)), 15), (265, 0, 295)).
    # In the box's frame the ray cuts the corner x = z = 0 at y = 100: in at (0, 100, e), out at (e, 100, 0),
    # e = L / sqrt(2); rotate_y maps a local point to (c x + s z, y, -s x + c z) (hittable.rs:386-415)
    e = L / np.sqrt(2.0)
    s, c = np.sin(np.radians(15.0)), np.cos(np.radians(15.0))
    to_world = lambda v: np.array([c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2]])
    mid = to_world(np.array([0.5 * e, 100.0, 0.5 * e])) + np.array([265.0, 0.0, 295.0])
    return mid, to_world(np.array([1.0, 0.0, -1.0]) / np.sqrt(2.0)), 200.0


@pytest.mark.parametrize("name", ["final", "media"])
def test_thin_chords_through_a_medium(rt, renderer, name):
    with _plain_twins():
        tw, _ = tf._final_world(rt, DENSE) if name == "final" else tf._cornell_world(rt, True, DENSE)
    w = World(name, WORLDS[name][0], tw.product, None, None, frozenset(tw.phase), tw)
    rays = _chord_rays(rt, _sphere_chord if name == "final" else _box_chord)
    ref = tw.oracle.hit(rays, SEED, 0)
    fog = is_phase(w, ref["mat"]) & (ref["hit"] != 0)
    print(f"{name}: chords in t {[c for c, _ in CHORDS]}, |d| {[l for _, l in CHORDS]}: oracle medium hits {fog.tolist()}, t {ref['t'].tolist()}")
    # the reference: a chord of 0.5e-4 in t is under the 0.0001 step whatever |d| is, one of 2e-4 over it
    assert fog.tolist() == [chord > 1e-4 for chord, _ in CHORDS]
    renderer.upload(tw.product)
    hits, alb = renderer.trace_rays(rays, seed=SEED, bounce=0, albedo=True)
    assert renderer.query_stats().invalid == 0 and renderer.query_stats().variant_features == w.variant
    print(f"{name}: device t {hits['t'].tolist()}, flags {hits['flags'].tolist()}")
    compare(rt, hits, alb, ref, w, f"{name} thin chords")


# ---- scene 7: the layouts of the query's nested walk ---------------------------------------------------
LAYOUT_FIELDS = ("t", "p", "n", "prim", "mat", "flags", "key_pixel", "key_sample")


def _assert_same_records(rt, got, want, label):
    hits, alb, occ = got
    for f in LAYOUT_FIELDS:
        assert hits[f].tobytes() == want[0][f].tobytes(), (label, f)
    solid = (hits["flags"] & rt.RT_HIT_MEDIUM) == 0      # inner of a medium's hit: rt_abi.h excepts it
    assert np.array_equal(hits["inner"][solid], want[0]["inner"][solid]), label
    assert np.array_equal(alb, want[1]) and np.array_equal(occ, want[2]), label


def _both(r, rays, rt):
    hits, alb = r.trace_rays(rays, seed=SEED, albedo=True)
    return hits, alb, r.trace_rays(rays, mode=rt.RT_QUERY_ANY, seed=SEED)


def _cluster_set(rt):
    w = world(rt, "scene7_cluster")
    s = ray_set(rt, "scene7_cluster")
    inside = (s.kind == oracle_rays.MIDPOINT) & (s.src_top == CLUSTER_TOP)
    print(f"scene7_cluster: {int(inside.sum())} origins are midpoints of the cluster's first and second hit")
    assert inside.sum() >= 100
    return w, s


def _run_layout(rt, w, s, variant=None, extra=0, accel=None):
    """The set's records (hits, albedo, occluded) and the query's stats on a fresh context."""
    r = rt.Renderer(0)
    try:
        if variant is not None:
            r.set_variant(*variant)
        if extra:
            r.set_option(rt.RT_OPT_EXTRA_FEATURES, extra)
        r.upload(w.product, rt.RT_ACCEL_SAH if accel is None else accel)
        got = _both(r, s.rays, rt)
        st = r.query_stats()
        assert st.invalid == 0 and st.variant_features == (4095 if extra else w.variant)
        return got, st
    finally:
        r.close()


def test_scene7_layouts_give_the_default_records(rt):
    """The final scene's query is laid out with SceneFacts.nested_stack_entries (26 entries against the
    trace kernels' 13). The same 1,000 rays, at least 100 of them starting inside a sphere of the
    cluster's instance, under the stack in scratch, f64 slabs, no TLAS in LDS, all three, and the
    all-features variant: the default's records, which are held to the oracle here and in
    test_caller_rays_match_the_oracle[scene7_cluster], byte for byte."""
    w, s = _cluster_set(rt)
    want, st = _run_layout(rt, w, s)
    assert st.slab32 == 1
    compare(rt, want[0], want[1], s.ref[0], w, "scene7_cluster default")
    for variant in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        got, st = _run_layout(rt, w, s, variant=variant)
        assert st.slab32 == variant[0]
        _assert_same_records(rt, got, want, f"set_variant{variant}")
    _assert_same_records(rt, _run_layout(rt, w, s, extra=4095)[0], want, "RT_OPT_EXTRA_FEATURES 4095")


@pytest.mark.parametrize("accel", ["LINEAR", "MEDIAN"])
def test_scene7_acceleration_structures_give_the_default_records(rt, accel):
    """The same rays over the two other acceleration structures: the default's (SAH) records byte for
    byte, `inner` on medium hits excepted.

    Scene 7's 400 ground boxes tile a grid, so a side of one coincides with a side of its neighbour and
    both rect tests accept exactly the same t (a rect rejects t > t_max only). Four of the set's rays
    (74, 732, 764, 778) end on such a side. When the query kept the record of the later test, as
    rt_render's casts do, SAH named boxes 253, 261, 141, 239 for them and LINEAR and MEDIAN 266, 263,
    163, 241, and this test failed on prim and inner alone; cast_interval now keeps, of two top-level
    records with the same t, the one later in rt_scene_soa.prims — the later entry of the list, which
    hit_hittables' loop keeps — under every structure."""
    w, s = _cluster_set(rt)
    want, _ = _run_layout(rt, w, s)
    got, _ = _run_layout(rt, w, s, accel=getattr(rt, "RT_ACCEL_" + accel))
    compare(rt, got[0], got[1], s.ref[0], w, f"scene7_cluster {accel}")
    differ = {f: np.flatnonzero(got[0][f] != want[0][f]) for f in ("prim", "inner")}
    for f in ("t", "p", "n", "mat", "flags", "key_pixel", "key_sample"):
        assert got[0][f].tobytes() == want[0][f].tobytes(), (accel, f)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), accel
    print(f"scene7_cluster {accel}: prim {want[0]['prim'][[74, 732, 764, 778]].tolist()} on the four shared sides; differs from SAH's on rays {differ['prim'].tolist()}, inner on {differ['inner'].tolist()}; "
          f"their oracle top {s.ref[0]['top'][differ['prim']].tolist()}, SAH prim {want[0]['prim'][differ['prim']].tolist()}, "
          f"{accel} prim {got[0]['prim'][differ['prim']].tolist()}")
    _assert_same_records(rt, got, want, f"RT_ACCEL_{accel}")
