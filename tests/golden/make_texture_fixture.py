#!/usr/bin/env python3
"""Expected texture values at the points of tests/texture_points.py, from the independent reference
tests/texture_reference.py (mpmath and exact rationals): tests/golden/texture_expected.npz.

A plane world's expectation needs no implementation at all: its rays land on the points exactly. A
carrier world's hit points are rounded, so the oracle's record supplies which material a ray ends on
and the point p (both go into the fixture; a GPU hit must reproduce them bit for bit before its
albedo is judged), and the reference evaluates the texture there: u and v from the carrier's own
geometry in mpmath, never from the oracle's u and v or albedo. The Perlin tables are read as data
from the product's HIP-free World.flatten().

Per world `w` the fixture holds w.code (one byte per ray: a texel index j * 7 + i, or one of the
codes of tests/texture_points.py), w.gray (the noise rays' values, in ray order), w.sha (the sha256
of the ray records the values belong to), and for a carrier world w.mat and w.p.

usage: python tests/golden/make_texture_fixture.py   (tests/test_texture_reference.py regenerates
the arrays and asserts them equal to the committed file)
"""
import ctypes
import os
import sys
from fractions import Fraction

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import oracle_binding as ob  # noqa: E402
from tests import texture_points as tp  # noqa: E402
from tests import texture_reference as tr  # noqa: E402

FIXTURE = tp.FIXTURE
MARGIN = 1e-9        # a sphere- or instance-borne image point whose u w or v h is nearer an integer is left out


def product_tables(rt, build, scene_seed=tp.SCENE_SEED):
    """The Perlin instances of a world, in the order its noise textures were made, from the product's
    flattened tables (rt_scene_soa.perlin_ranvec / perlin_perm), as texture_reference.Tables."""
    w = rt.World(scene_seed)
    build(w)
    soa = w.flatten()
    n = soa.n_perlin
    if n == 0:
        w.close()
        return [], None, None
    ranvec = np.ctypeslib.as_array(ctypes.cast(soa.perlin_ranvec, ctypes.POINTER(ctypes.c_double)), (n, 256, 3)).copy()
    perm = np.ctypeslib.as_array(ctypes.cast(soa.perlin_perm, ctypes.POINTER(ctypes.c_int32)), (n, 3, 256)).copy()
    w.close()
    return [tr.Tables(ranvec[i], perm[i]) for i in range(n)], ranvec, perm


def plane_expected(rt, tex, axis):
    s = tp.plane_set(tex, axis)
    code = np.full(len(s.pts), tp.CODE_UNPINNED, dtype=np.uint8)
    gray = []
    if tex == "checker":
        for i in np.flatnonzero(s.pinned):
            code[i] = tp.CODE_ODD if tr.checker_odd(s.pts[i]) else tp.CODE_EVEN
    elif tex == "image":
        f0, f1 = tp.FREE[axis]
        for i, p in enumerate(s.pts):
            u, v = tr.rect_uv(p[f0], p[f1], *tp.IMAGE_RECT)
            ti, tj = tr.image_texel(tp.IMG_W, tp.IMG_H, u, v)
            code[i] = tj * tp.IMG_W + ti
    else:
        tables = product_tables(rt, lambda w: tp.plane_world(w, tex, axis))[0][0]
        for i in np.flatnonzero(s.pinned):
            code[i] = tp.CODE_NOISE
            gray.append(tr.noise_value(tables, tp.NOISE_SCALES[tex], s.pts[i]))
    return {"code": code, "gray": np.array(gray, dtype=np.float64), "sha": tp.ray_sha(s.rays)}, {}


def _centre(geom, time):
    """hittable.rs:556-558 in exact rationals, rounded to doubles once."""
    c0, c1, t0, t1, _ = geom
    if tuple(c0) == tuple(c1):
        return np.array(c0)
    s = (Fraction(float(time)) - Fraction(t0)) / (Fraction(t1) - Fraction(t0))
    return np.array([float(Fraction(a) + s * (Fraction(b) - Fraction(a))) for a, b in zip(c0, c1)])


def _box_texel(p):
    """The instanced box's object-space face point from the world-space p (the inverse of
    hittable.rs:399-408 and :236, in mpmath): ((i, j), margins), or None next to a box edge."""
    with mpmath.workprec(tr.PREC):
        a = mpmath.mpf(tp.BOX_ANGLE) * mpmath.pi / 180
        s, c = mpmath.sin(a), mpmath.cos(a)
        q = [mpmath.mpf(float(p[k])) - mpmath.mpf(tp.BOX_OFFSET[k]) for k in range(3)]
        o = [c * q[0] - s * q[2], q[1], s * q[0] + c * q[2]]
        on = [k for k in range(3) if min(abs(o[k]), abs(o[k] - tp.BOX_MAX[k])) < MARGIN]
        if len(on) != 1:
            return None
        f0, f1 = tp.FREE[tp.PLANE_AXIS.index(on[0])]
        uw = o[f0] / tp.BOX_MAX[f0] * tp.IMG_W
        vh = (1 - o[f1] / tp.BOX_MAX[f1]) * tp.IMG_H
        i, j = min(int(mpmath.floor(uw)), tp.IMG_W - 1), min(int(mpmath.floor(vh)), tp.IMG_H - 1)
        return (i, j), (float(abs(uw - mpmath.nint(uw))), float(abs(vh - mpmath.nint(vh))))


def carrier_expected(rt, name):
    build, make_set = tp.CARRIER_WORLDS[name]
    rays, derived = make_set()
    tables = product_tables(rt, build)[0]
    world = ob.OracleWorld(tp.SCENE_SEED)
    carriers = build(world)
    rec = world.hit(rays, tp.QUERY_SEED, 0)
    world.close()
    n = len(rays)
    code = np.full(n, tp.CODE_MISS, dtype=np.uint8)
    gray, margins, left_out, judged_random = [], [], 0, 0
    for i in np.flatnonzero(rec["hit"] != 0):
        c, p = carriers[int(rec["mat"][i])], rec["p"][i]
        if c.tex == "metal":
            code[i] = tp.CODE_METAL
        elif c.tex == "ones":
            code[i] = tp.CODE_ONES
        elif c.tex == "checker":
            code[i] = tp.CODE_ODD if tr.checker_odd(p) else tp.CODE_EVEN
        elif c.tex == "noise":
            code[i] = tp.CODE_NOISE
            gray.append(tr.noise_value(tables[c.geom], tp.NOISE_CARRIER_SCALE, p))
        elif c.uv == "zero":                 # hittable.rs:452-462: u = v = 0
            ti, tj = tr.image_texel(tp.IMG_W, tp.IMG_H, 0.0, 0.0)
            assert (ti, tj) == (0, tp.IMG_H - 1)
            code[i] = tj * tp.IMG_W + ti
        elif c.uv == "rect_exact":
            obj = [Fraction(float(p[k])) - Fraction(tp.EXACT_OFFSET[k]) for k in range(3)]
            assert obj[1] == tp.INSTANCE_RECT[4] and all(Fraction(float(v)) == v for v in obj), p
            x0, x1, z0, z1, _ = tp.INSTANCE_RECT
            ti, tj = tr.image_texel(tp.IMG_W, tp.IMG_H, *tr.rect_uv(float(obj[0]), float(obj[2]), x0, x1, z0, z1))
            code[i] = tj * tp.IMG_W + ti
        else:
            if c.uv == "sphere":
                got = tr.sphere_texel(tp.IMG_W, tp.IMG_H, p, _centre(c.geom, rays["time"][i]), c.geom[4])
            else:
                got = _box_texel(p)
            if not derived[i]:
                judged_random += 1
            if got is None or (not derived[i] and min(got[1]) < MARGIN):
                code[i] = tp.CODE_UNPINNED
                left_out += 1
                continue
            if not derived[i]:
                margins.append(min(got[1]))
            code[i] = got[0][1] * tp.IMG_W + got[0][0]
    hit = rec["hit"] != 0
    arrays = {"code": code, "gray": np.array(gray, dtype=np.float64), "sha": tp.ray_sha(rays),
              "mat": rec["mat"].astype(np.uint8), "p": rec["p"][hit].copy()}
    report = {"left_out": left_out, "random_image_points": judged_random,
              "min_margin": min(margins) if margins else None,
              "per_carrier": {c.name: int((rec["mat"][hit] == m).sum()) for m, c in carriers.items()}}
    return arrays, report


def generate(rt):
    """(arrays as the fixture holds them, a report per world)."""
    arrays, report = {}, {}
    for tex in tp.PLANE_TEXTURES:
        for axis in range(3):
            a, r = plane_expected(rt, tex, axis)
            name = f"{tex}_{axis}"
            arrays.update({f"{name}.{k}": v for k, v in a.items()})
            report[name] = r
    for name in tp.CARRIER_WORLDS:
        a, r = carrier_expected(rt, name)
        arrays.update({f"{name}.{k}": v for k, v in a.items()})
        report[name] = r
    return arrays, report


if __name__ == "__main__":
    import __graft_entry__ as ge
    arrays, report = generate(ge.import_binding())
    np.savez_compressed(FIXTURE, **arrays)
    for name in tp.CARRIER_WORLDS:
        print(name, report[name])
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
