"""Worlds whose pixel value does not depend on which path was drawn, and their checks.

HIP-free: the builders issue constructor calls on whatever world they are given (a
tests/oracle_binding.py OracleWorld or TwinWorld: the same method names), the checks are
numpy. Every renderer that implements the reference must give these pixels to rounding, so
a kernel whose paths are not the oracle's (the f32 fast mode) can still be
held to the oracle per pixel:

- one-bounce worlds: one convex scatterer of albedo a under a constant sky bg. A sample is
  bg (miss) or a*bg (one bounce, then out), so j_c = (img_c/bg_c - 1)/(a_c - 1)*spp is the
  same integer in [0, spp] on the three channels. A re-hit of the surface just left gives
  a^2*bg, which moves j_c by another non-integer amount per channel.
- the furnace: every albedo is 1, so a sample is bg, or black for a path that never
  escapes (the reference has a few: trapped paths). j = (1 - img_c/bg_c)*spp is one integer.
- ID worlds: every primitive is an emitter of its own colour, so a pixel is the colour of
  the first hit. Interior pixels (3x3 pure over several oracle seeds) are seed-independent.
- a noise emitter: the first hit's Perlin value, bracketed by the oracle's neighbourhood.

tests/test_path_free_worlds.py proves on the oracle alone every condition the GPU tests
(tests/test_gpu_f32_exact.py) rely on.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

BG = (0.7, 0.8, 1.0)
ALBEDO = (0.5, 0.4, 0.3)
SEEDS = (1, 2, 3, 4)

# compiled kernel variants (csrc/scene_features.hpp)
SPHERES, RECTINST, MEDIA, FINAL, ALL = 0, 35, 103, 287, 4095


def camera24(look_from, look_at, vfov, aspect, vup=(0.0, 1.0, 0.0), aperture=0.0, focus_dist=10.0, time0=0.0,
             time1=1.0) -> np.ndarray:
    """The reference camera (camera.rs:18-56) as the 24 doubles OracleWorld.render takes."""
    lf, la, up = (np.asarray(x, dtype=np.float64) for x in (look_from, look_at, vup))
    h = np.tan(np.radians(vfov) / 2.0)
    vh = 2.0 * h
    vw = aspect * vh
    w = (lf - la) / np.linalg.norm(lf - la)
    u = np.cross(up, w)
    u /= np.linalg.norm(u)
    v = np.cross(w, u)
    hor, ver = u * (focus_dist * vw), v * (focus_dist * vh)
    llc = lf - hor * 0.5 - ver * 0.5 - w * focus_dist
    return np.concatenate([lf, llc, hor, ver, u, v, w, [aperture * 0.5, time0, time1]])


@dataclass
class Spec:
    """One world: build(w) issues the constructor calls; the view; the compiled variant it
    selects (features) and the RT_OPT_EXTRA_FEATURES bits that select it where the scene's
    own do not."""
    name: str
    build: Callable
    look_from: tuple
    look_at: tuple
    vfov: float
    W: int = 48
    H: int = 32
    spp: int = 8
    features: int = SPHERES
    extra: int = 0
    vup: tuple = (0.0, 1.0, 0.0)
    albedo: Optional[tuple] = ALBEDO     # one-bounce worlds: None = the glass sphere (a = 1, every pixel bg)
    owners: list = field(default_factory=list)   # ID worlds: (colour, class) per emitter colour
    min_share: float = 0.6               # ID worlds: interior share the oracle must reach
    n_spheres: int = 0                   # the big field: its sphere count

    def cam24(self):
        return camera24(self.look_from, self.look_at, self.vfov, self.W / self.H, self.vup)


# ---- one-bounce worlds ------------------------------------------------------------------------

def _mat(w, kind):
    if kind == "lambertian":
        return w.lambertian(w.solid(*ALBEDO))
    if kind == "metal":
        return w.metal(ALBEDO, 0.0)
    return w.dielectric(1.5)


GRAZE_UP = (0.5, 0.75 ** 0.5, 0.0)
GRAZE_FROM = (1000.05 * GRAZE_UP[0], 1000.05 * GRAZE_UP[1] - 1000.0, 0.0)


def one_bounce_worlds() -> list:
    shapes = {
        # name: (push(w, mat), look_from, look_at, vfov, variant, extra)
        "ground": (lambda w, m: w.push(w.sphere(m, (0.0, -1000.0, 0.0), 1000.0)),
                   (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, SPHERES, 0),
        "grazing": (lambda w, m: w.push(w.sphere(m, (0.0, -1000.0, 0.0), 1000.0)),
                    (0.0, 0.05, 0.0), (0.0, 0.05, -1.0), 20.0, SPHERES, 0),
        # the same incidence 30 degrees down the sphere from its top, where the hit points'
        # coordinates are ~500 and an f32 hit point lies up to ~3e-5 off the surface (near the top
        # the coordinate along the normal is small, and so is its rounding): the camera 0.05 off
        # the surface, looking along the tangent
        "grazing-far": (lambda w, m: w.push(w.sphere(m, (0.0, -1000.0, 0.0), 1000.0)),
                        GRAZE_FROM, (GRAZE_FROM[0], GRAZE_FROM[1], -1.0), 20.0, SPHERES, 0),
        "unit": (lambda w, m: w.push(w.sphere(m, (0.0, 0.0, 0.0), 1.0)),
                 (0.0, 0.5, 4.0), (0.0, 0.0, 0.0), 40.0, SPHERES, 0),
        "far_small": (lambda w, m: w.push(w.sphere(m, (600.0, 0.0, 800.0), 0.2)),
                      (600.0, 0.5, 803.0), (600.0, 0.0, 800.0), 10.0, SPHERES, 0),
        "r8.0": (lambda w, m: w.push(w.sphere(m, (1.0, 2.0, -3.0), 8.0)),
                 (1.0, 6.0, 27.0), (1.0, 2.0, -3.0), 40.0, SPHERES, 0),
        "r8.5": (lambda w, m: w.push(w.sphere(m, (1.0, 2.0, -3.0), 8.5)),
                 (1.0, 6.0, 27.0), (1.0, 2.0, -3.0), 40.0, SPHERES, 0),
        "moving": (lambda w, m: w.push(w.moving_sphere(m, (0.0, 0.0, 0.0), (0.0, 0.5, 0.0), 0.0, 1.0, 1.0)),
                   (0.0, 0.5, 5.0), (0.0, 0.25, 0.0), 40.0, SPHERES, 0),
        "xz_rect": (lambda w, m: w.push(w.xz_rect(m, -2.0, 2.0, -2.0, 2.0, 0.0)),
                    (1.0, 3.0, 6.0), (0.0, 0.0, 0.0), 40.0, RECTINST, 0),
        "rotbox": (lambda w, m: w.push(w.translate(w.rotate_y(w.box((0.0, 0.0, 0.0), (165.0, 330.0, 165.0), m), 15.0),
                                                   (265.0, 0.0, 295.0))),
                   (278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 20.0, RECTINST, 0),
        # a top-level box near the scene extent, on the final-scene variant (C4's ground boxes)
        "box1000": (lambda w, m: w.push(w.box((990.0, -10.0, -10.0), (1000.0, 300.0, 10.0), m)),
                    (1200.0, 150.0, 300.0), (995.0, 145.0, 0.0), 10.0, FINAL, 8),
    }
    out = []
    for name, (push, lf, la, vfov, feat, extra) in shapes.items():
        for kind in ("lambertian", "metal"):
            out.append(Spec(f"{name}-{kind}", (lambda w, push=push, kind=kind: push(w, _mat(w, kind))), lf, la, vfov,
                            features=feat, extra=extra))
            if name == "grazing-far":
                out[-1].vup, out[-1].W, out[-1].H = GRAZE_UP, 96, 64
    out.append(Spec("glass", lambda w: w.push(w.sphere(_mat(w, "glass"), (0.0, 0.0, 0.0), 1.0)),
                    (0.0, 0.5, 4.0), (0.0, 0.0, 0.0), 40.0, albedo=None))
    return out


def lattice_j(img, bg, a, spp, tol):
    """(ok, j): j the per-pixel count of one-bounce samples, ok where the three channels give
    that one integer in [0, spp] within tol. a = None (albedo 1): ok where the pixel is bg
    (relative tol / spp, the same scale), j = 0."""
    img = np.asarray(img, dtype=np.float64)
    bg = np.asarray(bg, dtype=np.float64)
    if a is None:
        ok = np.all(np.abs(img / bg - 1.0) * spp <= tol, axis=-1)
        return ok, np.zeros(img.shape[:-1], dtype=np.int64)
    jc = (img / bg - 1.0) / (np.asarray(a, dtype=np.float64) - 1.0) * spp
    j = np.rint(jc[..., 0])
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(jc - j[..., None]) <= tol, axis=-1) & (j >= 0) & (j <= spp)
    return ok, np.where(np.isfinite(j), j, -1).astype(np.int64)


def channel_j(img, bg, a, spp):
    """The three per-channel values of j at one pixel (failure messages)."""
    img, bg = np.asarray(img, dtype=np.float64), np.asarray(bg, dtype=np.float64)
    if a is None:
        return (img / bg - 1.0) * spp
    return (img / bg - 1.0) / (np.asarray(a, dtype=np.float64) - 1.0) * spp


def settled(js, value):
    """Pixels whose 3x3 neighbourhood has j == value in every image of js (several seeds)."""
    m = np.all(np.stack(js) == value, axis=0)
    return _erode(m)


def _erode(m):
    p = np.pad(m, 1, constant_values=False)
    out = np.ones_like(m)
    for dy in range(3):
        for dx in range(3):
            out &= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


# ---- the furnace ------------------------------------------------------------------------------

def _furnace(w, full):
    one = (1.0, 1.0, 1.0)
    white = w.lambertian(w.solid(*one))
    check = w.lambertian(w.checker(one, one))
    mirror = w.metal(one, 0.0)
    glass = w.dielectric(1.5)
    phase = w.isotropic(w.solid(*one))
    # nothing is tangent to anything else: every object floats >= 0.3 above the ground
    if full:
        w.push(w.sphere(check, (0.0, -1000.0, 0.0), 1000.0))
        w.push(w.sphere(white, (-3.2, 1.0, 0.0), 0.7))
        w.push(w.sphere(mirror, (-1.6, 1.0, 0.3), 0.7))
        w.push(w.sphere(glass, (0.0, 1.0, 0.6), 0.7))
        w.push(w.constant_medium(w.sphere(white, (1.6, 1.0, 0.3), 0.7), 0.8, phase))
        w.push(w.moving_sphere(white, (3.2, 0.9, 0.0), (3.2, 1.3, 0.0), 0.0, 1.0, 0.5))
        balls = w.bvh([w.sphere((white, mirror, glass)[i % 3], (0.45 * (i % 8), 0.45 * (i // 8), 0.2 * (i % 2)), 0.15)
                       for i in range(40)])
        w.push(w.translate(w.rotate_y(balls, 20.0), (-1.5, 2.2, -1.5)))
    else:
        w.push(w.xz_rect(check, -30.0, 30.0, -30.0, 30.0, 0.0))
        w.push(w.box((-3.6, 0.4, -0.5), (-2.6, 1.6, 0.5), white))
        w.push(w.box((-2.0, 0.4, -0.2), (-1.0, 1.6, 0.8), mirror))
        w.push(w.translate(w.rotate_y(w.box((0.0, 0.0, 0.0), (1.0, 1.4, 1.0), glass), 30.0), (-0.4, 0.4, 0.2)))
        w.push(w.constant_medium(w.box((1.2, 0.4, -0.3), (2.2, 1.6, 0.7), white), 0.8, phase))
        w.push(w.yz_rect(white, 0.4, 2.0, -1.5, 1.0, -4.5))
        w.push(w.xy_rect(mirror, -3.0, 3.0, 0.4, 2.5, -2.5))
    if full:     # a medium under instances, its boundary an instanced box: only the all-features variant holds that
        smoke = w.constant_medium(w.translate(w.rotate_y(w.box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), white), 15.0),
                                              (-0.5, 0.0, -0.5)), 1.0, phase)
        w.push(w.translate(w.rotate_y(smoke, 40.0), (2.6, 0.4, 2.0)))
    else:        # a top-level medium bounded by an instanced box
        w.push(w.constant_medium(w.translate(w.rotate_y(w.box((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), white), 55.0),
                                             (2.1, 0.4, 1.5)), 1.0, phase))


def furnace_world(full: bool = True) -> Spec:
    """Everything has albedo exactly 1. full: every primitive and material kind, media under
    instances (the all-features variant). Reduced: rects, boxes and box-bounded media (the
    media variant)."""
    return Spec("furnace" if full else "furnace-media", lambda w: _furnace(w, full), (1.0, 4.0, 11.0), (0.0, 1.0, 0.0),
                40.0, W=64, H=40, spp=16, features=ALL if full else MEDIA, albedo=(1.0, 1.0, 1.0))


def furnace_black(img, bg, spp, tol):
    """(ok, n_black): per pixel j = (1 - img_c/bg_c)*spp, the number of black samples, must be
    one integer in [0, spp] on the three channels; n_black its sum over the pixels."""
    jc = (1.0 - np.asarray(img, dtype=np.float64) / np.asarray(bg, dtype=np.float64)) * spp
    j = np.rint(jc[..., 0])
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(jc - j[..., None]) <= tol, axis=-1) & (j >= 0) & (j <= spp)
    return ok, int(np.where(np.isfinite(j), j, 0).sum())


# ---- ID worlds --------------------------------------------------------------------------------

def palette(n: int, bg=BG) -> list:
    """n exact f64 colours in (0, 1), pairwise >= 0.06 apart in L_inf (a 0.06 lattice, walked
    with a stride that scatters neighbours) and >= 0.05 from bg."""
    cols = []
    k = 0
    while len(cols) < n:
        idx = (k * 1789) % 4096
        k += 1
        assert k <= 4096, "palette exhausted"
        c = tuple(0.06 * (1 + ((idx >> s) & 15)) for s in (0, 4, 8))
        if max(abs(c[i] - bg[i]) for i in range(3)) >= 0.05:
            cols.append(c)
    return cols


class _Emitters:
    """Hands out palette colours and records which class owns each."""

    def __init__(self, w, n):
        self.w, self.cols, self.owners = w, palette(n), []

    def mat(self, cls):
        c = self.cols[len(self.owners)]
        self.owners.append((c, cls))
        return self.w.diffuse_light(self.w.solid(*c))

    def checker(self):
        c1 = self.cols[len(self.owners)]
        self.owners.append((c1, "checker even"))
        c2 = self.cols[len(self.owners)]
        self.owners.append((c2, "checker odd"))
        return self.w.diffuse_light(self.w.checker(c1, c2))


def _id_world(w, rects, inst_boxes, blas):
    """Emitters on a 4.8 x 3 stage seen from (1.5, 2, 6): the 3-D checker's cells are pi/10
    wide, so the stage is small enough for a cell to span ~10 pixels at 160 x 100."""
    e = _Emitters(w, 64)
    w.push(w.sphere(e.mat("large sphere"), (0.0, -1000.6, 0.0), 1000.0))
    w.push(w.sphere(e.checker(), (-1.6, 0.35, 0.3), 0.85))
    w.push(w.sphere(e.mat("large sphere"), (0.1, 0.2, 0.9), 0.55))
    for i in range(6):
        w.push(w.sphere(e.mat("small sphere"), (-0.6 + 0.42 * (i % 3), 1.25 + 0.42 * (i // 3), 0.0), 0.19))
    if rects:
        w.push(w.xy_rect(e.mat("xy rect"), 1.0, 1.8, 0.9, 1.7, -0.5))
        w.push(w.xz_rect(e.mat("xz rect"), 0.9, 1.9, 0.6, 1.6, -0.1))
        w.push(w.yz_rect(e.mat("yz rect"), -0.3, 0.7, 0.2, 1.4, 0.85))
        w.push(w.box((2.1, -0.4, 0.0), (2.7, 0.4, 0.6), e.mat("box")))
    if inst_boxes:
        w.push(w.translate(w.box((0.0, 0.0, 0.0), (0.5, 0.7, 0.5), e.mat("translated box")), (2.2, 0.8, -0.6)))
        w.push(w.translate(w.rotate_y(w.box((0.0, 0.0, 0.0), (0.5, 0.7, 0.5), e.mat("rotated box")), 30.0),
                           (-0.9, 1.5, -0.8)))
    if blas:
        ids = [w.sphere(e.mat("instanced-BVH sphere"), (0.44 * (i % 4), 0.44 * (i // 4), 0.1 * (i % 2)), 0.2)
               for i in range(12)]
        w.push(w.translate(w.rotate_y(w.bvh(ids), 20.0), (-2.9, 1.45, -0.3)))
    return e.owners


def _big_field(w, nx, nz):
    """nx x nz emitter spheres seen from above (more than 408 TLAS nodes: the spheres
    variant's partial-TLAS instantiation with the 32-bit stack). Neighbours overlap, so the
    discs tile the screen and most of a disc is interior."""
    e = _Emitters(w, nx * nz)
    for i in range(nx * nz):
        x, z = i % nx, i // nx
        w.push(w.sphere(e.mat("field sphere"), (x - 0.5 * (nx - 1), 0.05 * ((x * 3 + z * 5) % 4), z - 0.5 * (nz - 1)), 0.6))
    return e.owners


def id_worlds() -> list:
    """One emitter world per f32 instantiation (csrc/trace_f32_*.hip)."""
    def spec(name, feat, extra=0, **kw):
        s = Spec(name, None, (1.5, 2.0, 6.0), (-0.1, 0.55, 0.0), 28.0, W=160, H=100, spp=4, features=feat, extra=extra,
                 albedo=None)

        def build(w, s=s):
            s.owners = _id_world(w, **kw)
        s.build = build
        return s

    out = [spec("id-spheres", SPHERES, rects=False, inst_boxes=False, blas=False),
           spec("id-rectinst", RECTINST, rects=True, inst_boxes=True, blas=False),
           spec("id-media", MEDIA, extra=4 | 64, rects=True, inst_boxes=True, blas=False),
           spec("id-final", FINAL, rects=True, inst_boxes=False, blas=True),
           spec("id-all", ALL, rects=True, inst_boxes=True, blas=True)]
    nx, nz = 42, 26
    big = Spec("id-bigfield", None, (0.0, 60.0, 0.0), (0.0, 0.0, 0.0), 24.0, W=320, H=200, spp=2, features=SPHERES,
               albedo=None, vup=(0.0, 0.0, -1.0), min_share=0.3, n_spheres=nx * nz)

    def build_big(w):
        big.owners = _big_field(w, nx, nz)
    big.build = build_big
    return out + [big]


def interior(oracle_imgs) -> np.ndarray:
    """Pixels that, with their eight neighbours, are one single colour (to 1e-12) in every
    image of oracle_imgs (the union of several oracle seeds)."""
    imgs = np.stack(oracle_imgs)
    ref = imgs[0]
    H, W = ref.shape[:2]
    p = np.pad(imgs, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="constant", constant_values=np.nan)
    ok = np.ones((H, W), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            with np.errstate(invalid="ignore"):
                ok &= np.all(np.abs(p[:, dy:dy + H, dx:dx + W] - ref[None]) <= 1e-12, axis=(0, 3))
    return ok


def owner_counts(img, mask, owners) -> dict:
    """Interior pixels per class: a pixel belongs to the owner whose colour it is (1e-12)."""
    out = {}
    for c, cls in owners:
        n = int(np.sum(mask & np.all(np.abs(img - np.asarray(c)) <= 1e-12, axis=-1)))
        out[cls] = out.get(cls, 0) + n
    return out


def colours_owning(img, mask, owners) -> int:
    """How many of the owners' colours own at least one interior pixel."""
    px = img[mask]
    return sum(1 for c, _ in owners if np.any(np.all(np.abs(px - np.asarray(c)) <= 1e-12, axis=-1)))


# ---- the noise emitter ------------------------------------------------------------------------

NOISE_WINDOW = 5      # the bracket's neighbourhood (NOISE_WINDOW x NOISE_WINDOW); see test_path_free_worlds.py
NOISE_PAD = 1e-3


def noise_world() -> Spec:
    """A sphere that emits the Perlin marble texture (texture.rs noise, scale 4), seen from 0.6
    off its surface at vfov 15 so that it fills the frame: the turbulence's seventh octave has
    a wavelength of 1/64, and a pixel must be small against it for a pixel mean to lie between
    its neighbours'. (The whole r = 2 sphere at vfov 40 from z = 5 left 142-162 of 9,320 pixels
    outside a 5x5 bracket, 63-80 outside 7x7; this view leaves none, at 5x5.)"""
    def build(w):
        w.push(w.sphere(w.diffuse_light(w.noise(4.0)), (0.0, 0.0, 0.0), 2.0))
    return Spec("noise-emitter", build, (0.3, 0.2, 2.6), (0.0, 0.0, 0.0), 15.0, W=160, H=100, spp=4, features=FINAL,
                albedo=None)


def noise_on_sphere(oracle_imgs) -> np.ndarray:
    """Pixels all of whose samples hit the sphere in every seed: the marble is grey and the
    background is not, so those are the pixels with r == g == b."""
    imgs = np.stack(oracle_imgs)
    return np.all((np.abs(imgs[..., 0] - imgs[..., 1]) <= 1e-12) & (np.abs(imgs[..., 1] - imgs[..., 2]) <= 1e-12), axis=0)


def noise_bracket(oracle_img, on_sphere, window=NOISE_WINDOW, pad=NOISE_PAD):
    """(lo, hi, valid): per pixel and channel the min and max of the oracle's window x window
    neighbourhood, widened by pad; valid where the whole neighbourhood lies on the sphere
    (on_sphere: the mask of pixels that are not background in any oracle seed)."""
    r = window // 2
    H, W = oracle_img.shape[:2]
    p = np.pad(oracle_img, ((r, r), (r, r), (0, 0)), mode="edge")
    m = np.pad(on_sphere, r, constant_values=False)
    lo = np.full(oracle_img.shape, np.inf)
    hi = np.full(oracle_img.shape, -np.inf)
    valid = np.ones((H, W), dtype=bool)
    for dy in range(window):
        for dx in range(window):
            s = p[dy:dy + H, dx:dx + W]
            lo, hi = np.minimum(lo, s), np.maximum(hi, s)
            valid &= m[dy:dy + H, dx:dx + W]
    return lo - pad, hi + pad, valid
