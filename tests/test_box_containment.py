"""The box invariant of the lowering (csrc/flatten.cpp), checked on the tables the kernel walks,
without a GPU: every node box bounds what the primitive tests below it accept.

"Closest hit is independent of the hierarchy" rests on that. For every generated world
(tests/generated_worlds.py), every accel mode and the camera shutter the world is rendered with,
and for the eight preset scenes, this walks the tables of rt_world_flatten from tlas_root through
nodes and leaves, prim_refs, prims and instances (and an instance's BLAS in object space), takes
points on the surface each leaf primitive's hit test accepts, and requires every point inside
every box above it. No tolerance beyond the padding the boxes carry.

The table layouts are restated here from include/rt/rt_scene.h as numpy dtypes.

What it guards against: with boxes taken from the reference's bounding_box this test fails on
the worlds neg_radius ("primitive 35 (kind 0, p = [-3.0, 3.0, 0.0, -1.3, ...]) has the accepted
point [-1.7, 3.0, 0.0] outside its ancestor box node 0 child 1: lo [-1.80, 0.0999, -0.4001] hi
[12.80, 2.80, 2.30]"), shutters and camera_time_inside ("primitive 0 (kind 1, p = [-5.5, 0.5,
-1.5, 0.3, ..., 0.25, 0.75]) has the accepted point [-5.2, 0.0, -1.5] outside its ancestor box
node 0 child 1: lo [-5.80, 0.19997, -1.80] hi [6.00, 1.80003, 1.80]") and rotations (a rotate_y
over a negative radius: a node box with lo.y 0.892 above hi.y 0.108), each a wrong image on the
GPU (L_inf 0.97, 0.90, 0.048 and 0.22 against the oracle), and only under SAH: LINEAR's and
MEDIAN's top-level nodes are unbounded.
"""
import ctypes

import numpy as np
import pytest

from tests import generated_worlds as gw

PRIM = np.dtype([("kind", "<i4"), ("mat", "<i4"), ("a", "<i4"), ("b", "<i4"), ("p", "<f8", (10,))])
INSTANCE = np.dtype([("n_ops", "<i4"), ("child_kind", "<i4"), ("child", "<i4"), ("pad", "<i4"),
                     ("op_kind", "<i4", (4,)), ("op", "<f8", (4, 3))])
NODE = np.dtype([("lo0", "<f4", (3,)), ("hi0", "<f4", (3,)), ("lo1", "<f4", (3,)), ("hi1", "<f4", (3,)),
                 ("child", "<i4", (2,)), ("pad", "<i4", (2,))])
SPHERE, MOVING, XY, XZ, YZ, BOX, INST, MEDIUM = range(8)
OP_TRANSLATE, OP_ROTATE_Y = 0, 1
CHILD_PRIM, CHILD_BVH = 0, 1
ACCELS = {"sah": 0, "linear": 1, "median": 2}


def test_restated_layouts_have_the_headers_sizes():
    assert (PRIM.itemsize, INSTANCE.itemsize, NODE.itemsize) == (96, 128, 64)


def _unit_vectors():
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    v += [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]
    v += [(1, 2, -2), (-3, 1, 2), (2, -1, 3), (0, 3, 4), (-4, 0, 3)]
    a = np.array(v, dtype=np.float64)
    return a / np.linalg.norm(a, axis=1)[:, None]


UNIT = _unit_vectors()


class Tables:
    def __init__(self, soa):
        def table(ptr, n, dt):
            if not n:
                return np.zeros(0, dt)
            return np.frombuffer(ctypes.string_at(ptr, n * dt.itemsize), dtype=dt).copy()
        self.prims = table(soa.prims, soa.n_prims, PRIM)
        self.refs = table(soa.prim_refs, soa.n_prim_refs, np.dtype("<i4"))
        self.nodes = table(soa.nodes, soa.n_nodes, NODE)
        self.instances = table(soa.instances, soa.n_instances, INSTANCE)
        self.root = soa.tlas_root
        self.n_tlas_nodes = soa.n_tlas_nodes
        self.n_checked = 0


class Walk:
    """Collects failures as text; times: the ray times a moving sphere is sampled at."""

    def __init__(self, t: Tables, times, label):
        self.t, self.times, self.label, self.failures = t, times, label, []
        self.n_points = 0
        self.n_boxes = 0

    def points_of(self, pi):
        """Points the hit test of primitive pi accepts, in the space pi lives in."""
        q = self.t.prims[pi]
        k, p = int(q["kind"]), q["p"]
        if k == SPHERE:
            return p[0:3] + abs(p[3]) * UNIT
        if k == MOVING:
            # MovingSphere::center (hittable.rs:556-558): c0 + (c1 - c0) * ((time - t0) / (t1 - t0))
            return np.concatenate([p[0:3] + p[5:8] * ((tm - p[8]) / (p[9] - p[8])) + abs(p[3]) * UNIT for tm in self.times])
        if k in (XY, XZ, YZ):
            a = np.array([p[0], p[1], 0.5 * (p[0] + p[1]), 0.75 * p[0] + 0.25 * p[1]])
            b = np.array([p[2], p[3], 0.5 * (p[2] + p[3]), 0.25 * p[2] + 0.75 * p[3]])
            if not (p[0] <= p[1] and p[2] <= p[3]):
                return np.zeros((0, 3))     # an inverted rect accepts nothing
            aa, bb = [g.ravel() for g in np.meshgrid(a, b)]
            kk = np.full_like(aa, p[4])
            return np.stack({XY: (aa, bb, kk), XZ: (aa, kk, bb), YZ: (kk, aa, bb)}[k], axis=1)
        if k == BOX:
            return np.array([[p[0 + 3 * i], p[1 + 3 * j], p[2 + 3 * l]] for i in (0, 1) for j in (0, 1) for l in (0, 1)])
        if k == MEDIUM:
            return self.points_of(int(q["a"]))      # its boundary
        assert k == INST, k
        inst = self.t.instances[int(q["a"])]
        if int(inst["child_kind"]) == CHILD_PRIM:
            pts = self.points_of(int(inst["child"]))
        else:   # the BLAS in object space: its own boxes must hold there
            pts = self.walk(int(inst["child"]), [], f"BLAS of instance {int(q['a'])}")
        for i in range(int(inst["n_ops"]) - 1, -1, -1):   # object -> world, innermost op first
            o = inst["op"][i]
            if int(inst["op_kind"][i]) == OP_TRANSLATE:
                pts = pts + o
            else:
                s, c = o[0], o[1]
                pts = np.stack([c * pts[:, 0] + s * pts[:, 2], pts[:, 1], -s * pts[:, 0] + c * pts[:, 2]], axis=1)
        return pts

    def walk(self, ref, boxes, where):
        """All points below ref, each checked against `boxes` (the boxes above ref in this walk)."""
        if ref < 0:
            code = ~ref
            first, count = code >> 5, code & 31
            out = [np.zeros((0, 3))]
            for j in range(first, first + count):
                pi = int(self.t.refs[j])
                pts = self.points_of(pi)
                self.n_points += len(pts)
                for (lo, hi, name) in boxes:
                    self.n_boxes += 1
                    bad = ~(np.all(pts >= lo, axis=1) & np.all(pts <= hi, axis=1))
                    if bad.any():
                        self.failures.append(
                            f"{self.label}, {where}: primitive {pi} (kind {int(self.t.prims[pi]['kind'])}, "
                            f"p = {self.t.prims[pi]['p'][:10].tolist()}) has the accepted point {pts[bad][0].tolist()} "
                            f"outside its ancestor box {name}: lo {lo.tolist()} hi {hi.tolist()}")
                out.append(pts)
            return np.concatenate(out)
        nd = self.t.nodes[ref]
        out = []
        for c, (lo, hi) in enumerate(((nd["lo0"], nd["hi0"]), (nd["lo1"], nd["hi1"]))):
            box = (lo.astype(np.float64), hi.astype(np.float64), f"node {ref} child {c}")
            out.append(self.walk(int(nd["child"][c]), boxes + [box], where))
        return np.concatenate(out)


def check_world(world, accel, times, label):
    t = Tables(world.flatten(accel))
    w = Walk(t, times, label)
    w.walk(t.root, [], "TLAS")
    assert not w.failures, f"{len(w.failures)} points outside a box; the first: {w.failures[0]}"
    return t, w


def _times(case):
    return (case.time[0], 0.5 * (case.time[0] + case.time[1]), case.time[1])


@pytest.mark.parametrize("accel", list(ACCELS))
@pytest.mark.parametrize("case", gw.SUPPORTED, ids=[c.name for c in gw.SUPPORTED])
def test_generated_world_boxes_bound_what_their_primitives_accept(rt, case, accel):
    b = gw.build(rt, case)
    assert b.n_top >= 24
    t, w = check_world(b.tw.product, ACCELS[accel], _times(case), f"{case.name} ({accel})")
    assert w.n_points > 0
    if accel == "sah":     # the point of >= 24 items: boxes gate the walk
        assert t.n_tlas_nodes > 0 and w.n_boxes > 0
        blas = [int(i["child"]) for i in t.instances if int(i["child_kind"]) == CHILD_BVH]
        assert all(r >= 0 for r in blas), "an instanced BVH of one leaf: no BLAS box is exercised"


@pytest.mark.parametrize("accel", list(ACCELS))
@pytest.mark.parametrize("scene_id", range(8))
def test_preset_scene_boxes_bound_what_their_primitives_accept(rt, scene_id, accel):
    world = rt.World(1).build_scene(scene_id)
    _, w = check_world(world, ACCELS[accel], (0.0, 0.5, 1.0), f"scene {scene_id} ({accel})")
    assert w.n_points > 0


def test_no_supported_world_is_refused(rt):
    """The supported family keeps to what the lowering takes (chains of <= 4 ops, no instance in a
    medium boundary): the share refused is zero, in every accel mode, so no case hides behind one."""
    refused = []
    for case in gw.SUPPORTED:
        for name, accel in ACCELS.items():
            try:
                gw.build(rt, case).tw.product.flatten(accel)
            except rt.RTError as e:
                refused.append((case.name, name, str(e)))
    assert not refused, refused


def test_a_moving_sphere_without_a_shutter_is_refused_at_the_constructor(rt):
    """MovingSphere::center divides by t1 - t0: t0 == t1 (or a non-finite one) has no centre and
    no box. RT_ERR_INVALID with a message; the world stays usable."""
    w = rt.World(1)
    m = w.lambertian(w.solid(0.5, 0.5, 0.5))
    for t0, t1 in ((0.5, 0.5), (0.0, float("nan")), (float("inf"), 1.0)):
        with pytest.raises(rt.RTError, match="RT_ERR_INVALID.*t0 and t1"):
            w.moving_sphere(m, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), t0, t1, 0.5)
    w.push(w.moving_sphere(m, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 1.0, 0.0, 0.5))
    check_world(w, 0, (0.0, 0.5, 1.0), "one moving sphere")


@pytest.mark.parametrize("case", gw.BVH_CASES, ids=[c.name for c in gw.BVH_CASES])
def test_bvh_over_unbounded_children_is_refused_with_a_message_or_lowered(rt, case):
    """rt_world_bvh over a child whose reference box does not bound it: RT_ERR_UNSUPPORTED naming
    the node and the child, the same in every accel mode; a world that is lowered holds the box
    invariant like any other (tests/test_gpu_generated_worlds.py then holds it to the oracle)."""
    outcomes = set()
    for name, accel in ACCELS.items():
        b = gw.build(rt, case)
        try:
            check_world(b.tw.product, accel, _times(case), f"{case.name} ({name})")
            outcomes.add("lowered")
        except rt.RTError as e:
            assert "RT_ERR_UNSUPPORTED" in str(e) and "rt_world_bvh node" in str(e) and "child" in str(e), str(e)
            outcomes.add("refused")
    assert len(outcomes) == 1, outcomes
    expect = {"bvh_neg_radius": "refused", "bvh_narrow_shutter": "refused", "bvh_rotated_neg_radius": "lowered",
              "bvh_wide_shutter": "lowered"}
    assert outcomes == {expect[case.name]}
