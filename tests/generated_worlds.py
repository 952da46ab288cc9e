"""Seeded twin worlds that sample the constructor ABI (rt_world_*) where the hand-built worlds of
the suite do not: negative radii, shutters that do not cover the camera's, cameras with another
time range, refraction indices and fuzz beside the presets', noise scales, rotations around the
whole circle on every primitive kind, translations by zero, chains of 1-4 ops, media of every
boundary kind and of densities over three decades, cameras inside a medium and inside glass,
every texture on every material and primitive that takes one, and cameras on both sides of the
f32-slab limit (2 * pad_extent, csrc/launch_plan.cpp).

Pure Python over tests/oracle_binding.TwinWorld: every world is built by the same calls in the
product and in the oracle. Nothing here needs a GPU. Every world has at least 24 top-level items
(the flattener makes a list of up to 8 one leaf, so a smaller world has no node box at all), and
every instanced BVH more than 8 leaves (so its BLAS has nodes too).

Two families:
  SUPPORTED   constructions the lowering supports; none of them may be refused
  BVH_CASES   rt_world_bvh over children whose reference bounding box does not bound them: the
              reference culls by those boxes, so each is either refused (RT_ERR_UNSUPPORTED at
              flatten) or rendered as the oracle renders it — nothing else

build(rt, case, skip=...) leaves out the primitives a case tags (its `finding`): the oracle's
image with and without them shows that the view looks at them.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Tuple

import numpy as np

from tests import oracle_binding as ob

W, H, SPP = 32, 24, 4            # the size every generated world is rendered at


@dataclass
class Case:
    name: str
    seed: int
    make: Callable                      # make(b: Builder) -> None
    look_from: Tuple[float, float, float]
    look_at: Tuple[float, float, float]
    bg: Tuple[float, float, float] = (0.7, 0.8, 1.0)
    vfov: float = 40.0
    aperture: float = 0.1
    focus: float = 10.0
    time: Tuple[float, float] = (0.0, 1.0)      # the camera's (time0, time1)
    finding: bool = False                       # holds primitives tagged "finding": build(skip=) can leave them out


class Builder:
    """A TwinWorld plus the case's bookkeeping: top-level pushes are counted, tagged primitives can
    be left out, and the build's time range follows the camera's when that leaves [0, 1]."""

    def __init__(self, rt, case: Case, skip=()):
        self.rt, self.case, self.skip = rt, case, frozenset(skip)
        self.tw = ob.TwinWorld(rt, case.seed)
        self.rng = np.random.default_rng(case.seed)
        self.n_top = 0
        lo, hi = min(case.time), max(case.time)
        if lo < 0.0 or hi > 1.0:    # the boxes are built for [0, 1] unless told otherwise (rt_abi.h)
            self.tw.product.set_build_option(rt.RT_BUILD_TIME0, lo)
            self.tw.product.set_build_option(rt.RT_BUILD_TIME1, hi)

    def __getattr__(self, name):
        return getattr(self.tw, name)

    def push(self, hid, tag=None):
        if tag is not None and tag in self.skip:
            return
        self.tw.push(hid)
        self.n_top += 1

    def u(self, a, b):
        return float(self.rng.uniform(a, b))


def synthetic_image(h, w, seed):
    """A small RGB8 array: a gradient with seeded noise, so neighbouring texels differ."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([40 + 200 * x / max(w - 1, 1), 30 + 210 * y / max(h - 1, 1), 255 - 25 * ((x + y) % 8)], axis=2)
    return np.clip(img + rng.integers(-20, 21, size=img.shape), 0, 255).astype(np.uint8)


def _filler(b: Builder, n, x0=-5.5, z0=-3.0, dx=1.0, per_row=12, y=0.35, r=0.3):
    """n small spheres on a grid, materials cycling: the bulk that gives the TLAS its nodes."""
    mats = [b.lambertian(b.solid(0.7, 0.3, 0.2)), b.metal((0.8, 0.8, 0.9), 0.1), b.dielectric(1.5),
            b.lambertian(b.checker((0.1, 0.2, 0.6), (0.9, 0.9, 0.8)))]
    for i in range(n):
        c = (x0 + dx * (i % per_row), y, z0 + 1.1 * (i // per_row))
        b.push(b.sphere(mats[i % 4], c, r))


# ---- the supported family ---------------------------------------------------------------------

def _neg_radius(b: Builder):
    """Finding 1: spheres of radius < 0 alone (no ground sphere whose box would cover them) and
    concentric inside a positive one, in lambertian, metal and dielectric."""
    floor = b.lambertian(b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    lam = b.lambertian(b.solid(0.8, 0.2, 0.2))
    met = b.metal((0.9, 0.7, 0.3), 0.0)
    glass = b.dielectric(1.5)
    mats = (lam, met, glass)
    for i in range(24):     # unit-spaced, two rows
        b.push(b.sphere(mats[i % 3], (float(i % 12), 0.5, 1.5 * (i // 12)), 0.4))
    for k, (outer, inner) in enumerate(((glass, glass), (glass, met), (glass, lam), (lam, lam))):
        c = (1.5 + 3.0 * k, 2.2, 0.7)
        b.push(b.sphere(outer, c, 0.6))
        b.push(b.sphere(inner, c, -0.5))          # the hollow-glass idiom
    b.push(b.xz_rect(floor, -6.0, 18.0, -4.0, 7.0, 0.0))
    for mat, c, r in ((glass, (14.0, 3.0, 0.0), -1.4), (met, (14.0, 3.0, 3.5), -1.2), (lam, (-3.0, 3.0, 0.0), -1.3),
                      (glass, (-3.0, 3.0, 3.5), -1.2)):
        b.push(b.sphere(mat, c, r), tag="finding")


def _shutters(b: Builder):
    """Finding 2: moving spheres whose shutter lies inside, equals, surrounds and is disjoint from
    the camera's [0, 1]; their centres extrapolate beyond the hull of the two shutter centres."""
    lam = b.lambertian(b.solid(0.8, 0.3, 0.1))
    met = b.metal((0.8, 0.8, 0.9), 0.5)
    glass = b.dielectric(1.3)
    floor = b.lambertian(b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))
    shutters = ((0.25, 0.75), (0.0, 1.0), (-1.0, 2.0), (2.0, 3.0), (0.4, 0.6), (1.0, 0.0))
    for i in range(30):
        t0, t1 = shutters[i % 6]
        x, z = -5.5 + (i % 12), -1.5 + 1.5 * (i // 12)
        covers = min(t0, t1) <= 0.0 and max(t0, t1) >= 1.0
        b.push(b.moving_sphere((lam, met, glass)[i % 3], (x, 0.5, z), (x + 0.2 * (i % 2), 1.5, z), t0, t1, 0.3),
               tag=None if covers else "finding")
    b.push(b.xz_rect(floor, -8.0, 8.0, -4.0, 5.0, -3.0))


def _camera_time(time):
    def make(b: Builder):
        """Moving spheres with the presets' shutter [0, 1] (and two others) under a camera whose
        (time0, time1) is not (0, 1)."""
        lam = b.lambertian(b.solid(0.2, 0.6, 0.3))
        met = b.metal((0.7, 0.6, 0.5), 1.0)
        for i in range(26):
            t0, t1 = ((0.0, 1.0), (0.0, 1.0), (0.3, 0.5), (-2.0, 4.0))[i % 4]
            x, z = -6.0 + (i % 13), -1.0 + 2.0 * (i // 13)
            b.push(b.moving_sphere(lam if i % 2 else met, (x, 0.4, z), (x, 1.4, z + 0.3), t0, t1, 0.35),
                   tag="finding" if (t0, t1) != (-2.0, 4.0) else None)
        b.push(b.sphere(b.lambertian(b.noise(0.3)), (0.0, -50.0, 0.0), 49.0))
    return make


def _materials(b: Builder):
    """Refraction indices beside 1.5 (below 1, exactly 1, diamond), fuzz up to and above 1 (the
    reference clamps nothing), noise scales beside 4 (one below 1)."""
    irs = (0.5, 1.0, 1.3, 1.5, 2.4)
    fuzzes = (0.0, 0.5, 1.0, 1.7)
    scales = (0.3, 4.0, 11.0, 0.9)
    k = 0
    for row, mats in enumerate(([b.dielectric(ir) for ir in irs], [b.metal((0.9, 0.8, 0.6), f) for f in fuzzes],
                                [b.lambertian(b.noise(s)) for s in scales])):
        for j in range(10):
            b.push(b.sphere(mats[j % len(mats)], (-5.0 + 1.1 * j, 0.5, -2.0 + 2.0 * row), 0.5 if j % 2 else 0.42))
            k += 1
    b.push(b.sphere(b.lambertian(b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), (0.0, -1000.0, 0.0), 1000.0))
    b.push(b.xz_rect(b.diffuse_light(b.solid(4.0, 4.0, 4.0)), -3.0, 3.0, -2.0, 2.0, 6.0))


def _prims_with(b: Builder, mat_of, x0):
    """Every primitive kind once per texture: sphere, moving sphere, the three rects, a box."""
    texs = (lambda: b.checker((0.8, 0.2, 0.2), (0.2, 0.2, 0.9)), lambda: b.noise(2.5),
            lambda: b.image(synthetic_image(5, 7, b.case.seed)), lambda: b.image(synthetic_image(1, 1, b.case.seed + 1)))
    for t, tex in enumerate(texs):
        z = -3.0 + 2.0 * t
        b.push(b.sphere(mat_of(tex()), (x0, 0.6, z), 0.6))
        b.push(b.moving_sphere(mat_of(tex()), (x0 + 1.5, 0.5, z), (x0 + 1.5, 0.9, z), 0.0, 1.0, 0.5))
        b.push(b.xy_rect(mat_of(tex()), x0 + 2.3, x0 + 3.5, 0.0, 1.2, z))
        b.push(b.xz_rect(mat_of(tex()), x0 + 3.8, x0 + 5.0, z - 0.6, z + 0.6, 0.3))
        b.push(b.yz_rect(mat_of(tex()), 0.0, 1.2, z - 0.6, z + 0.6, x0 + 5.6))
        b.push(b.box((x0 + 6.0, 0.0, z - 0.5), (x0 + 7.0, 1.0, z + 0.5), mat_of(tex())))
        b.push(b.translate(b.rotate_y(b.box((0.0, 0.0, 0.0), (0.8, 0.8, 0.8), mat_of(tex())), 30.0), (x0 + 7.6, 0.0, z - 0.4)))


def _textures_lambertian(b: Builder):
    _prims_with(b, b.lambertian, -4.5)
    b.push(b.xz_rect(b.lambertian(b.image(synthetic_image(5, 7, 3))), -8.0, 8.0, -6.0, 6.0, -0.01))


def _textures_light(b: Builder):
    _prims_with(b, b.diffuse_light, -4.5)
    b.push(b.xz_rect(b.lambertian(b.solid(0.7, 0.7, 0.7)), -8.0, 8.0, -6.0, 6.0, -0.01))


def _blob(b: Builder, mat, c, n=10, r=0.45):
    """n overlapping spheres around c: a boundary (or an instanced cluster) whose BVH has nodes."""
    return b.bvh([b.sphere(mat, (c[0] + 0.3 * math.cos(2.4 * i) * (i % 3), c[1] + 0.12 * (i % 4), c[2] + 0.3 * math.sin(2.4 * i)), r)
                  for i in range(n)])


def _media(b: Builder):
    """Media bounded by a sphere, a box, an instanced box and a bare BVH, with checker, noise and
    image textures on the isotropic phase, densities over three decades; the camera sits inside a
    thin medium."""
    white = b.lambertian(b.solid(0.73, 0.73, 0.73))
    texs = (lambda: b.checker((0.9, 0.3, 0.3), (0.3, 0.3, 0.9)), lambda: b.noise(0.9),
            lambda: b.image(synthetic_image(5, 7, 21)), lambda: b.solid(0.1, 0.1, 0.1))
    densities = (0.02, 0.2, 2.0, 20.0)
    for t, tex in enumerate(texs):
        z = -3.0 + 2.0 * t
        for k, d in enumerate(densities):
            x = -5.0 + 2.6 * k
            phase = b.isotropic(tex())
            boundary = (b.sphere(white, (x, 0.7, z), 0.7),
                        b.box((x - 0.6, 0.0, z - 0.6), (x + 0.6, 1.2, z + 0.6), white),
                        b.translate(b.rotate_y(b.box((0.0, 0.0, 0.0), (1.1, 1.3, 1.1), white), 20.0 + 50.0 * t), (x - 0.5, 0.0, z - 0.5)),
                        _blob(b, white, (x, 0.5, z)))[(k + t) % 4]
            b.push(b.constant_medium(boundary, densities[(k + t) % 4], phase))
    for i in range(8):
        b.push(b.sphere(white, (-5.0 + 1.5 * i, 0.3, 5.0), 0.3))
    b.push(b.constant_medium(b.sphere(white, (0.0, 4.0, 11.0), 3.0), 0.05, b.isotropic(b.solid(0.9, 0.9, 1.0))))   # around the camera
    b.push(b.sphere(b.lambertian(b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), (0.0, -1000.0, 0.0), 1000.0))
    b.push(b.xz_rect(b.diffuse_light(b.solid(5.0, 5.0, 5.0)), -4.0, 4.0, -3.0, 3.0, 7.0))


ANGLES = (0.0, 90.0, -90.0, 135.0, 180.0, 270.0, 400.0, 33.3, -17.5, 721.25, 89.999, 1e-7)


def _rotations(b: Builder):
    """rotate_y around the circle on boxes, rects, spheres (one of negative radius) and moving
    spheres (one with a shutter inside the camera's); translate by zero; chains of 1-4 ops; an
    instanced BVH of 12 spheres."""
    lam = b.lambertian(b.checker((0.8, 0.6, 0.2), (0.2, 0.2, 0.3)))
    met = b.metal((0.8, 0.8, 0.8), 0.05)
    glass = b.dielectric(1.5)
    light = b.diffuse_light(b.solid(3.0, 3.0, 3.0))
    zero = (0.0, 0.0, 0.0)
    for i, ang in enumerate(ANGLES):
        off = (-5.5 + 1.0 * i, 0.0, -2.0)
        kind = i % 4
        child = (b.box((0.0, 0.0, 0.0), (0.6, 0.9, 0.4), lam),
                 b.xy_rect(met, 0.0, 0.7, 0.0, 0.9, 0.2),
                 b.sphere(glass, (0.4, 0.5, 0.1), -0.4 if i % 8 == 2 else 0.4),
                 b.moving_sphere(lam, (0.3, 0.4, 0.0), (0.3, 0.8, 0.2), *((0.25, 0.75) if i % 8 == 3 else (0.0, 1.0)), 0.3))[kind]
        b.push(b.translate(b.rotate_y(child, ang), off))                                  # 2 ops
    for i, ang in enumerate(ANGLES):
        x = -5.5 + 1.0 * i
        kind = i % 4
        if kind == 0:      # 1 op
            b.push(b.rotate_y(b.yz_rect(lam, 0.0, 0.8, x, x + 0.6, 0.0 + 0.1 * i), ang if i < 6 else 0.0))
        elif kind == 1:    # translate by zero
            b.push(b.translate(b.box((x, 0.0, 0.6), (x + 0.6, 0.7, 1.2), met), zero))
        elif kind == 2:    # 3 ops
            b.push(b.translate(b.rotate_y(b.translate(b.xz_rect(light if i == 2 else lam, -0.3, 0.3, -0.3, 0.3, 0.0), zero), ang), (x, 1.6, 1.0)))
        else:              # 4 ops
            b.push(b.translate(b.rotate_y(b.translate(b.rotate_y(b.box((-0.2, 0.0, -0.2), (0.2, 0.6, 0.2), lam), ang), (0.3, 0.0, 0.0)), -ang), (x, 0.0, 2.4)))
    balls = b.bvh([b.sphere((lam, met, glass)[i % 3], (0.45 * (i % 6), 0.25 + 0.5 * (i // 6), 0.2 * (i % 2)), 0.22 if i != 5 else 0.2)
                   for i in range(12)])
    b.push(b.translate(b.rotate_y(balls, 135.0), (2.0, 0.0, 4.0)))
    b.push(b.translate(balls, zero))
    b.push(b.sphere(b.lambertian(b.solid(0.5, 0.5, 0.5)), (0.0, -1000.0, 0.0), 1000.0))


def _inside_glass(b: Builder):
    """The camera sits inside a glass sphere (every primary ray leaves through it)."""
    _filler(b, 26)
    b.push(b.sphere(b.dielectric(1.5), b.case.look_from, 1.5))
    b.push(b.sphere(b.lambertian(b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), (0.0, -1000.0, 0.0), 1000.0))


def _extent_eight(b: Builder):
    """A world whose pad_extent is exactly 8 (its farthest box face), for the cameras on both
    sides of the f32-slab limit |camera| <= 2 * pad_extent."""
    _filler(b, 24, y=0.5, r=0.4)
    b.push(b.box((-8.0, -0.5, -8.0), (8.0, 0.0, 8.0), b.lambertian(b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9)))))
    b.push(b.moving_sphere(b.metal((0.9, 0.9, 0.9), 0.0), (0.0, 2.0, 0.0), (0.5, 2.5, 0.0), 0.0, 1.0, 0.8))


PAD_EXTENT_EIGHT = 8.0

SUPPORTED = [
    Case("neg_radius", 101, _neg_radius, (5.5, 5.0, 17.0), (5.5, 1.5, 1.0), vfov=55.0, finding=True),
    Case("shutters", 102, _shutters, (0.0, 3.0, 13.0), (0.0, 0.8, 0.0), vfov=45.0, finding=True),
    Case("camera_time_outside", 103, _camera_time((-0.5, 1.5)), (0.0, 4.0, 14.0), (0.0, 0.8, 0.0), vfov=45.0,
         time=(-0.5, 1.5), finding=True),
    Case("camera_time_inside", 104, _camera_time((0.2, 0.6)), (0.0, 4.0, 14.0), (0.0, 0.8, 0.0), vfov=45.0, time=(0.2, 0.6)),
    Case("materials", 105, _materials, (0.0, 5.0, 12.0), (0.0, 0.5, 0.0), bg=(0.2, 0.25, 0.3)),
    Case("textures_lambertian", 106, _textures_lambertian, (0.0, 7.0, 11.0), (0.0, 0.3, 0.0), vfov=50.0),
    Case("textures_light", 107, _textures_light, (0.0, 7.0, 11.0), (0.0, 0.3, 0.0), vfov=50.0, bg=(0.0, 0.0, 0.0)),
    Case("media", 108, _media, (0.0, 4.0, 11.0), (0.0, 0.5, 0.0), vfov=50.0, bg=(0.1, 0.1, 0.15)),
    Case("rotations", 109, _rotations, (0.0, 5.0, 11.0), (0.0, 0.5, 0.5), vfov=50.0),
    Case("inside_glass", 110, _inside_glass, (0.0, 3.0, 9.0), (0.0, 0.3, 0.0)),
    # |camera| 16.5 > 2 * 8: the f64-slab fallback; 15.5 (+ the lens' 0.15) < 16: the f32 slabs
    Case("camera_beyond_slab32", 111, _extent_eight, (0.0, 16.5 * 0.6, 16.5 * 0.8), (0.0, 0.5, 0.0), vfov=35.0),
    Case("camera_within_slab32", 111, _extent_eight, (0.0, 15.5 * 0.6, 15.5 * 0.8), (0.0, 0.5, 0.0), vfov=35.0),
]

FINDINGS = [c for c in SUPPORTED if c.finding]
# every world with a primitive the reference's box does not bound (a negative radius, or a shutter
# that does not cover the camera's), tagged or not
UNBOUNDED_BY_REFERENCE = FINDINGS + [c for c in SUPPORTED if c.name in ("camera_time_inside", "rotations")]


# ---- rt_world_bvh over children the reference's boxes do not bound: refused or equal -------------

def _bvh_case(children):
    def make(b: Builder):
        lam = b.lambertian(b.solid(0.8, 0.3, 0.2))
        glass = b.dielectric(1.5)
        ids = [b.sphere(lam if i % 2 else glass, (float(i) - 5.5, 0.5, 0.0), 0.4) for i in range(12)]
        b.push(b.bvh(ids + children(b, lam, glass)))
        b.push(b.xz_rect(b.lambertian(b.checker((0.2, 0.3, 0.1), (0.9, 0.9, 0.9))), -8.0, 8.0, -4.0, 4.0, 0.0))
    return make


BVH_CASES = [
    Case("bvh_neg_radius", 201, _bvh_case(lambda b, lam, glass: [b.sphere(glass, (8.0, 3.0, 0.0), -0.9)]),
         (0.0, 3.0, 14.0), (0.0, 1.0, 0.0), vfov=50.0),
    Case("bvh_narrow_shutter", 202,
         _bvh_case(lambda b, lam, glass: [b.moving_sphere(lam, (-7.0, 0.5, 1.0), (-7.0, 1.5, 1.0), 0.25, 0.75, 0.5)]),
         (0.0, 3.0, 14.0), (0.0, 1.0, 0.0), vfov=50.0),
    # a rotate_y's box is the hull of its child's rotated corners, which un-inverts it: bounded
    Case("bvh_rotated_neg_radius", 203,
         _bvh_case(lambda b, lam, glass: [b.rotate_y(b.sphere(lam, (6.0, 2.0, 0.0), -0.8), 30.0)]),
         (0.0, 3.0, 14.0), (0.0, 1.0, 0.0), vfov=50.0),
    # a shutter around the camera's: the reference's hull bounds every centre
    Case("bvh_wide_shutter", 204,
         _bvh_case(lambda b, lam, glass: [b.moving_sphere(lam, (-7.0, 0.5, 1.0), (-7.0, 1.5, 1.0), -1.0, 2.0, 0.5)]),
         (0.0, 3.0, 14.0), (0.0, 1.0, 0.0), vfov=50.0),
]


def build(rt, case: Case, skip=()) -> Builder:
    b = Builder(rt, case, skip)
    case.make(b)
    return b


def camera(rt, case: Case, width=W, height=H):
    return rt.camera_new(case.look_from, case.look_at, (0.0, 1.0, 0.0), case.vfov, width / height, case.aperture,
                         case.focus, case.time[0], case.time[1])


def cam24(cam) -> np.ndarray:
    v = []
    for f in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w"):
        v += list(getattr(cam, f))
    return np.array(v + [cam.lens_radius, cam.time0, cam.time1])


def oracle_render(rt, case: Case, skip=(), threads=0, width=W, height=H, spp=SPP):
    b = build(rt, case, skip)
    return b.tw.oracle.render(cam24(camera(rt, case, width, height)), case.bg, width, height, spp, threads=threads)
