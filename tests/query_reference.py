"""Reference side of the ray-query tests (test_camera_rays.py, test_gpu_trace_rays.py). Nothing here
calls rt_trace_rays.

closest_hit. A numpy restatement of hit_hittables(list, ray, t_min, t_max) for worlds of top-level
static spheres and axis-aligned rects (tests/features_reference.py's primitive tuples): oracle.c's
sphere_hit and rect_hit over the list in order, each with the ray's own t_min and t_max = the closest
hit so far, then the record of the winner (point, normal against the ray, front flag). Beside it the
margin of every decision the reference took for the ray — how far each discriminant, each root or
plane distance from the two interval ends, each rect coordinate from its edges and each pair of
accepted hits from one another stayed from zero — so a test can assert that no ray's classification
turns on less than the comparison tolerance.

caller_rays. The seeded set of 1,000 rays the GPU test traces through a SIMPLE world: origins in a box
around the scene and inside its spheres, unnormalised directions, and per-ray intervals in seven
classes: the cast's own (0.001, inf); t_max just short of the first hit (the hit must go, whatever
lies behind it must not be found either); t_max just past it; t_min just past it (the second hit
must be found); a window around the second hit; a negative t_min (hits behind the origin); and a
finite far t_max. "Just" is a relative 1e-4. A candidate whose margin is under MARGIN is drawn
again, so the set holds 1,000 rays that the tolerance can judge; tests/test_camera_rays.py asserts
the margins of the set it gets.
"""
import numpy as np

T_MIN = 0.001
MARGIN = 1e-6          # every decision of the reference is at least this far from turning
N_RAYS = 1000
JUST = 1e-4


def _scaled(x, ref):
    """|x| relative to 1 + |ref|: the comparison's own scale (1e-9 absolute plus relative)."""
    return np.abs(x) / (1.0 + np.abs(ref))


def closest_hit(prims, o, d, t_min, t_max):
    """o, d (n, 3), t_min, t_max (n,). Returns a dict: t (inf: a miss), p, n (zeros on a miss), front,
    index (the list index of the winner, -1), hits (tests that accepted) and margin (n,)."""
    n = o.shape[0]
    best_t = np.array(t_max, dtype=np.float64).copy()
    best_n = np.zeros((n, 3))
    best_i = np.full(n, -1)
    best_front = np.zeros(n, dtype=bool)
    hits = np.zeros(n, dtype=np.int64)
    margin = np.full(n, np.inf)
    accepted = []   # per primitive (hit mask, t)
    a = (d * d).sum(-1)
    with np.errstate(all="ignore"):
        for j, prim in enumerate(prims):
            if prim[0] == "sphere":
                c, r = np.array(prim[1], dtype=np.float64), float(prim[2])
                oc = o - c
                half_b = (oc * d).sum(-1)
                cc = (oc * oc).sum(-1) - r * r
                disc = half_b * half_b - a * cc
                # the discriminant against its own terms
                margin = np.minimum(margin, np.abs(disc) / (half_b * half_b + np.abs(a * cc) + 1e-300))
                sq = np.sqrt(np.where(disc >= 0, disc, 0.0))
                r0, r1 = (-half_b - sq) / a, (-half_b + sq) / a
                ok0 = ~((r0 < t_min) | (best_t < r0))
                ok1 = ~((r1 < t_min) | (best_t < r1))
                hit = (disc >= 0) & (ok0 | ok1)
                t = np.where(ok0, r0, r1)
                for root in (r0, r1):   # each root against the caller's two interval ends
                    m = np.minimum(_scaled(root - t_min, root), np.where(np.isfinite(t_max), _scaled(root - t_max, root), np.inf))
                    margin = np.where(disc >= 0, np.minimum(margin, m), margin)
                nrm = (o + t[:, None] * d - c) / r
            else:
                _, axis, a0, a1, b0, b1, k, _ = prim
                ka, aa, ba = ((2, 0, 1), (1, 0, 2), (0, 1, 2))[axis]
                t = (k - o[:, ka]) / d[:, ka]
                x = o[:, aa] + t * d[:, aa]
                y = o[:, ba] + t * d[:, ba]
                hit = ~((t < t_min) | (t > best_t)) & ~((x < a0) | (x > a1) | (y < b0) | (y > b1))
                margin = np.minimum(margin, np.abs(d[:, ka]) / np.sqrt(a))   # not parallel to the plane
                m = np.minimum(_scaled(t - t_min, t), np.where(np.isfinite(t_max), _scaled(t - t_max, t), np.inf))
                edge = np.minimum(np.minimum(np.abs(x - a0), np.abs(x - a1)), np.minimum(np.abs(y - b0), np.abs(y - b1)))
                margin = np.minimum(margin, np.minimum(m, edge))
                nrm = np.zeros((n, 3))
                nrm[:, ka] = 1.0
            front = (d * nrm).sum(-1) < 0.0
            nrm = np.where(front[:, None], nrm, -nrm)
            accepted.append((hit, t))
            best_t = np.where(hit, t, best_t)
            best_n = np.where(hit[:, None], nrm, best_n)
            best_i = np.where(hit, j, best_i)
            best_front = np.where(hit, front, best_front)
            hits += hit
        # accepted hits apart from one another: the closest is unambiguous
        for i in range(len(accepted)):
            for j in range(i + 1, len(accepted)):
                both = accepted[i][0] & accepted[j][0]
                margin = np.where(both, np.minimum(margin, _scaled(accepted[i][1] - accepted[j][1], accepted[i][1])), margin)
    any_hit = best_i >= 0
    t = np.where(any_hit, best_t, np.inf)
    p = np.where(any_hit[:, None], o + np.where(any_hit, best_t, 0.0)[:, None] * d, 0.0)
    nn = np.where(any_hit[:, None], best_n, 0.0)
    return dict(t=t, p=p, n=nn, front=any_hit & best_front, index=best_i, hits=hits, margin=margin)


def _candidates(prims, rng, m):
    """m candidate rays: origins in a box around the scene or inside a sphere, unnormalised directions."""
    spheres = [p for p in prims if p[0] == "sphere"]
    o = rng.uniform(-2.5, 2.5, size=(m, 3)) + np.array([0.0, 0.5, -0.5])
    inside = rng.random(m) < 0.3
    which = rng.integers(0, len(spheres), size=m)
    c = np.array([spheres[w][1] for w in which], dtype=np.float64)
    r = np.array([spheres[w][2] for w in which], dtype=np.float64)
    off = rng.normal(size=(m, 3))
    off = off / np.linalg.norm(off, axis=-1, keepdims=True) * (r * rng.uniform(0.05, 0.8, size=m))[:, None]
    o = np.where(inside[:, None], c + off, o)
    d = rng.normal(size=(m, 3))
    d = d / np.linalg.norm(d, axis=-1, keepdims=True) * rng.uniform(0.4, 2.5, size=m)[:, None]
    # aim most rays at the scene's middle so that hits and second hits are common
    aim = rng.random(m) < 0.6
    target = rng.uniform(-1.2, 1.2, size=(m, 3)) + np.array([0.0, 0.0, -1.2])
    to = target - o
    to = to / np.linalg.norm(to, axis=-1, keepdims=True) * np.linalg.norm(d, axis=-1, keepdims=True)
    d = np.where((aim & ~inside)[:, None], to, d)
    return o, d


def caller_rays(prims, seed=20261021):
    """(o, d, t_min, t_max, cls) of the N_RAYS-ray set for a primitive list; cls 0..6 as the module
    docstring lists the interval classes."""
    rng = np.random.default_rng(seed)
    out = [np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64)]
    while out[0].shape[0] < N_RAYS:
        m = 2048
        o, d = _candidates(prims, rng, m)
        base = closest_hit(prims, o, d, np.full(m, T_MIN), np.full(m, np.inf))
        t1 = base["t"]
        has = np.isfinite(t1)
        second = closest_hit(prims, o, d, np.where(has, t1 * (1.0 + JUST), T_MIN), np.full(m, np.inf))["t"]
        cls = rng.integers(0, 7, size=m)
        cls = np.where(has, cls, np.where(cls < 5, 0, cls))                   # classes 1-4 need a first hit,
        cls = np.where((cls == 4) & ~np.isfinite(second), 3, cls)             # class 4 a second one
        t_min = np.full(m, T_MIN)
        t_max = np.full(m, np.inf)
        t_max = np.where(cls == 1, t1 * (1.0 - JUST), t_max)
        t_max = np.where(cls == 2, t1 * (1.0 + JUST), t_max)
        t_min = np.where(cls == 3, t1 * (1.0 + JUST), t_min)
        t_min = np.where(cls == 4, second * (1.0 - JUST), t_min)
        t_max = np.where(cls == 4, second * (1.0 + JUST), t_max)
        t_min = np.where(cls == 5, -rng.uniform(0.5, 6.0, size=m), t_min)
        t_max = np.where(cls == 6, rng.uniform(0.5, 6.0, size=m), t_max)
        keep = (t_min <= t_max) & (closest_hit(prims, o, d, t_min, t_max)["margin"] > MARGIN) & (base["margin"] > MARGIN)
        for k, v in enumerate((o, d, t_min, t_max, cls)):
            out[k] = np.concatenate([out[k], v[keep]])
    return tuple(v[:N_RAYS] for v in out)


def as_rays(RAY, o, d, t_min, t_max, time=0.0, first_key=0):
    """RAY records (rtiow_amd.RAY) of a set; key (first_key + i, 0)."""
    rays = np.zeros(o.shape[0], dtype=RAY)
    rays["o"], rays["d"], rays["t_min"], rays["t_max"], rays["time"] = o, d, t_min, t_max, time
    rays["key_pixel"] = first_key + np.arange(o.shape[0])
    return rays
