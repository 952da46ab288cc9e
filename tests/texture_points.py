"""Worlds, points and rays for the texture comparison (tests/texture_reference.py): pure numpy and
`fractions`, seeded and deterministic; nothing here sees an oracle or a GPU result.

Plane worlds. plane_world(tw, tex, axis) is eight rects of one axis plane (axis 0: XY, 1: XZ, 2: YZ) at
the plane constants K, all carrying one texture (Lambertian on even entries of K, DiffuseLight on odd
ones). A ray runs along the plane's normal from one unit before the plane (k - 1 is exact for every k
in K, checked), so t = (k - (k - 1)) / 1 = 1 and p = o + 1 * d: nothing rounds and the ray lands on
the point itself, whatever implements the rect. The interval (0.75, 1.25) keeps the other seven
planes out (they are 0.5 apart or more). One world holds one axis and one texture because a ray
parallel to a rect whose plane it lies in gets t = 0 / 0 there, which hittable.rs:309-320 accepts (a
NaN fails every rejection test): with lattice coordinates next to plane constants that cannot be
avoided across axes, and two textures in one plane would tie.

Point classes. See NOISE_CLASSES, CHECKER_CLASSES and IMAGE_CLASSES; a point's plane coordinate is
the plane constant, the classes shape its two free coordinates. The classes named `unpinned` leave
the domain in which the textures are the reference's (a coordinate of 2^25 or more: 64 p passes i32;
|10 p_i| or |scale z| of 2^20 pi / 2 or more: the sine's reduction): they are compared GPU against
oracle only.

Carrier worlds. spheres_world and nested_world hold the other carriers of a texture's inputs: a
sphere (poles, seam), a negative radius, moving spheres, a rect and a box under
translate(rotate_y(.)), and constant media; see their docstrings. Their hit points are rounded, so
the expectation is taken at the oracle's p (tests/golden/make_texture_fixture.py).
"""
import hashlib
import os
from collections import namedtuple
from fractions import Fraction

import numpy as np

RAY = np.dtype([("o", "<f8", (3,)), ("d", "<f8", (3,)), ("time", "<f8"), ("t_min", "<f8"), ("t_max", "<f8"),
                ("key_pixel", "<u4"), ("key_sample", "<u4")])

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "texture_expected.npz")
SCENE_SEED = 7
K = (0.0, -0.5, 3.0, 255.0, 256.0, -256.25, 1000.0, 1.1)     # 1.1: not dyadic, and 1.1 - 1 is exact (Sterbenz)
EXTENT = 2.0 ** 41                                            # the noise / checker rects span +-EXTENT
EVEN, ODD = (0.2, 0.3, 0.1), (0.9, 0.9, 0.9)
NOISE_SCALES = {"noise4": 4.0, "noise01": 0.1, "noiseneg": -2.5}
PLANE_TEXTURES = ("checker", "noise4", "noise01", "noiseneg", "image")
PLANE_AXIS = (2, 1, 0)                                        # axis -> the coordinate the plane fixes
FREE = ((0, 1), (0, 2), (1, 2))                               # axis -> the record's (u, v) coordinates
IMG_W, IMG_H = 7, 5
IMAGE_RECT = (-1.5, 2.0, -0.75, 1.75)                         # a0, a1, b0, b1: 3.5 x 2.5, so u * 7 and v * 5 round
SIN_DOMAIN = 2.0 ** 20 * (np.pi / 2)                          # rt_numerics.h: the sine is accurate below it
M_LAST = 2 ** 19                                              # the last multiple of pi inside it
COORD_LIMIT = 2.0 ** 25                                       # from here 64 p passes i32

# pi to 100 digits (public), as a rational: the nearest double to m pi without mpmath
PI = Fraction(int("31415926535897932384626433832795028841971693993751058209749445923078164062862089986280348253421170679"),
              10 ** 100)


QUERY_SEED = 5                                                # the constant media's keyed draw, on every side

# an expected value's code, one byte per ray: a texel index j * IMG_W + i below 35, or
CODE_EVEN, CODE_ODD, CODE_NOISE, CODE_METAL, CODE_ONES, CODE_MISS, CODE_UNPINNED = 100, 101, 200, 210, 211, 220, 255


def image():
    """A 7 x 5 image whose 35 texels all differ in every channel pair."""
    j, i = np.mgrid[0:IMG_H, 0:IMG_W]
    return np.stack([10 + 35 * i, 20 + 50 * j, (37 * i + 11 * j + 5) % 256], axis=-1).astype(np.uint8)


def ray_sha(rays):
    """The sha256 of a set's ray records: the fixture's values belong to these rays and to no others."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(rays).tobytes()).digest(), dtype=np.uint8).copy()


def expected_albedo(code, gray):
    """The (n, 3) albedo a fixture's codes and noise values state, and which rays they judge (all but
    CODE_UNPINNED). A texel's colour is texture.rs:65-72's three f64 products (1 / 255) * byte."""
    code = np.asarray(code)
    out = np.zeros((len(code), 3))
    texel = code < IMG_W * IMG_H
    colours = (np.float64(1.0) / np.float64(255.0)) * image().reshape(-1, 3).astype(np.float64)
    out[texel] = colours[code[texel]]
    out[code == CODE_EVEN], out[code == CODE_ODD] = EVEN, ODD
    out[code == CODE_METAL], out[code == CODE_ONES] = METAL, 1.0
    assert int((code == CODE_NOISE).sum()) == len(gray)
    out[code == CODE_NOISE] = np.asarray(gray)[:, None]
    return out, code != CODE_UNPINNED


def judge(albedo, arrays, name, scale_z, classes, cls, label):
    """albedo against the fixture's expectation: exact for every code but the noise's, whose bar is
    2^-53 (4096 + 4 |scale z|) (derived in tests/texture_reference.py); the largest error per class is
    printed. Returns the largest noise error as a share of its bar."""
    want, judged = expected_albedo(arrays[f"{name}.code"], arrays[f"{name}.gray"])
    code = arrays[f"{name}.code"]
    noise = code == CODE_NOISE
    exact = judged & ~noise
    assert np.array_equal(albedo[exact], want[exact]), \
        f"{label}: albedo differs from the reference on rays {np.flatnonzero(exact & (albedo != want).any(1))[:10]}"
    share = 0.0
    if noise.any():
        assert (albedo[noise, 0] == albedo[noise, 1]).all() and (albedo[noise, 0] == albedo[noise, 2]).all()
        err = np.abs(albedo[noise, 0] - want[noise, 0])
        bar = 2.0 ** -53 * (4096.0 + 4.0 * np.abs(scale_z[noise]))
        for ci in np.unique(cls[noise]):
            m = cls[noise] == ci
            print(f"{label} {classes[ci]}: max |albedo - reference| = {err[m].max():.3e} over {int(m.sum())} points "
                  f"({(err[m] / bar[m]).max():.4f} of the bar)")
        worst = int(np.argmax(err / bar))
        assert (err <= bar).all(), (label, np.flatnonzero(noise)[worst], err[worst], bar[worst])
        share = float((err / bar).max())
    return share


def plane_world(tw, tex, axis):
    """Eight rects of one axis plane carrying `tex`, pushed in K's order (material handles 1, 2)."""
    if tex == "checker":
        t = tw.checker(EVEN, ODD)
    elif tex == "image":
        t = tw.image(image())
    else:
        t = tw.noise(NOISE_SCALES[tex])
    mats = (tw.lambertian(t), tw.diffuse_light(t))
    a0, a1, b0, b1 = IMAGE_RECT if tex == "image" else (-EXTENT, EXTENT, -EXTENT, EXTENT)
    rect = (tw.xy_rect, tw.xz_rect, tw.yz_rect)[axis]
    for i, k in enumerate(K):
        tw.push(rect(mats[i & 1], a0, a1, b0, b1, k))
    return tw


def _ulps(x, n):
    """x moved by n units in the last place (n an int array or scalar)."""
    x = np.asarray(x, dtype=np.float64)
    n = np.broadcast_to(np.asarray(n), x.shape)
    out = x.copy()
    for step in range(1, int(np.abs(n).max(initial=0)) + 1):
        out = np.where(n >= step, np.nextafter(out, np.inf), np.where(n <= -step, np.nextafter(out, -np.inf), out))
    return out


def _rng(*key):
    return np.random.default_rng([20261021, *key])


# ---- noise ------------------------------------------------------------------------------------------
NOISE_CLASSES = ("uniform", "lattice", "half", "minus_one", "wrap", "period", "octave_plane", "magnitude", "unpinned")
PER_CLASS = 32        # per axis: 96 per class and texture, 768 pinned points per texture


def _nudged(rng, base):
    """base, or base +- 1 ulp, or base +- 2^-30, in equal shares."""
    how = rng.integers(0, 5, size=base.shape)
    out = np.where(how == 1, _ulps(base, 1), np.where(how == 2, _ulps(base, -1), base))
    return np.where(how == 3, base + 2.0 ** -30, np.where(how == 4, base - 2.0 ** -30, out))


def _noise_free(rng, cls, n, z_col):
    """(n, 2) free coordinates of one class; z_col: which column is the point's z (None on an XY plane)."""
    if cls == "uniform":
        return rng.uniform(-8, 8, (n, 2))
    if cls == "lattice":                      # fraction 0 and 1 - 2^-53 through two smoothings
        return _nudged(rng, rng.integers(-6, 7, (n, 2)).astype(np.float64))
    if cls == "half":
        return rng.integers(-6, 6, (n, 2)) + 0.5
    if cls == "minus_one":                    # floor -1, index 255
        return np.where(rng.random((n, 2)) < 0.1, rng.choice([-1.0, -2.0 ** -60], (n, 2)), rng.uniform(-1, 0, (n, 2)))
    if cls == "wrap":
        base = rng.choice([255.0, 256.0, 257.0], (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
        return np.where(rng.random((n, 2)) < 0.5, _nudged(rng, base), base + rng.uniform(-1, 1, (n, 2)))
    if cls == "period":                       # pairs p, p + 256 e_i, both exact: rows 2 i and 2 i + 1
        p = np.round(rng.uniform(-4, 4, (n // 2, 2)) * 2.0 ** 30) / 2.0 ** 30
        q = p.copy()
        col = rng.integers(0, 2, n // 2)
        q[np.arange(n // 2), col] += 256.0 * rng.choice([-1.0, 1.0], n // 2)
        return np.stack([p, q], axis=1).reshape(n, 2)
    if cls == "octave_plane":                 # m / 64 +- tiny: the last octave crosses a lattice plane
        base = rng.integers(-512, 513, (n, 2)) / 64.0
        tiny = rng.choice([1, -1, 2, -2], (n, 2))
        out = np.where(rng.random((n, 2)) < 0.5, _ulps(base, tiny), base + tiny * 2.0 ** -40)
        out[:, 1] = np.where(rng.random(n) < 0.5, rng.uniform(-8, 8, n), out[:, 1])
        return out
    if cls == "magnitude":                    # 1e3, 1e5, just under 2^25 (64 p stays inside i32); z stays at 1e5
        mag = rng.choice([1e3, 1e5, COORD_LIMIT], (n, 2))
        val = np.where(mag == COORD_LIMIT, COORD_LIMIT - 1.0 - rng.uniform(0, 64, (n, 2)), mag * rng.uniform(0.5, 1, (n, 2)))
        if z_col is not None:
            val[:, z_col] = np.where(val[:, z_col] > 1e5, 1e5 * rng.uniform(0.5, 1, n), val[:, z_col])
        return val * rng.choice([-1.0, 1.0], (n, 2))
    if cls == "unpinned":                     # a coordinate of 2^25 and more; |scale z| beyond the sine's domain
        val = COORD_LIMIT * 2.0 ** rng.uniform(0, 15, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
        if z_col is not None:
            half = np.arange(n) % 2 == 0      # every other point: only z is large, the coordinates stay below 2^25
            val[half, 1 - z_col] = rng.uniform(-8, 8, int(half.sum()))
            val[half, z_col] = rng.uniform(5e5, 3e7, int(half.sum())) * rng.choice([-1.0, 1.0], int(half.sum()))
        return val
    raise ValueError(cls)


# ---- checker ----------------------------------------------------------------------------------------
CHECKER_CLASSES = ("uniform", "near_pi_small", "near_pi_domain", "near_pi_last", "switch", "zero", "unpinned")


def nearest_to_m_pi(m):
    """The double nearest m pi (float() of a Fraction rounds correctly)."""
    return float(m * PI)


def _tenth(a):
    """A double p with fl(10 p) == a, or NaN where the spacing of 10 p skips a."""
    a = np.asarray(a, dtype=np.float64)
    p = a / 10.0
    out = np.full(a.shape, np.nan)
    for n in (0, 1, -1, 2, -2):
        q = _ulps(p, n)
        out = np.where(np.isnan(out) & (10.0 * q == a), q, out)
    return out


def _near_m_pi(rng, m, n, limit=np.inf):
    """n coordinates p with 10 p = the double nearest m pi moved by -3..3 ulp (m drawn from `m`), |10 p| <= limit."""
    out = np.empty(0)
    while out.size < n:
        mm = rng.choice(m, n) * rng.choice([-1, 1], n)
        a = _ulps(np.array([nearest_to_m_pi(int(v)) for v in mm]), rng.integers(-3, 4, n))
        p = _tenth(a)
        out = np.concatenate([out, p[~np.isnan(p) & (np.abs(10.0 * p) <= limit)]])
    return out[:n]


def _checker_free(rng, cls, n):
    other = rng.uniform(-8, 8, n)
    if cls == "uniform":
        return rng.uniform(-8, 8, (n, 2))
    if cls == "near_pi_small":
        hard = _near_m_pi(rng, np.arange(1, 101), n)
    elif cls == "near_pi_domain":             # over the whole claimed domain |10 p| <= 2^20 pi / 2
        hard = _near_m_pi(rng, np.arange(1, M_LAST + 1), n, SIN_DOMAIN)
        other = np.where(rng.random(n) < 0.5, _near_m_pi(rng, np.arange(1, M_LAST + 1), n, SIN_DOMAIN), other)
    elif cls == "near_pi_last":               # its last few thousand multiples, the last twenty all present
        m = np.concatenate([np.arange(M_LAST - 3000, M_LAST - 19), np.repeat(np.arange(M_LAST - 19, M_LAST + 1), 150)])
        hard = _near_m_pi(rng, m, n, SIN_DOMAIN)
    elif cls == "switch":                     # rt_sin_sign's fast path ends at |x| = 65536; 20860 pi < 65536 < 20861 pi
        edge = _tenth(_ulps(np.full(16, 65536.0), np.arange(-8, 8)))
        hard = np.concatenate([edge[~np.isnan(edge)], _near_m_pi(rng, np.array([20859, 20860, 20861, 20862]), n)])[:n]
        hard = hard * rng.choice([-1.0, 1.0], n)
    elif cls == "zero":                       # a factor exactly 0: sin(+-0) = +-0, the product is not < 0
        hard = np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
        other = np.where(rng.random(n) < 0.5, _near_m_pi(rng, np.arange(1, 1001), n), other)
    elif cls == "unpinned":                   # beyond the sine's domain
        hard = _near_m_pi(rng, np.unique(np.round(2.0 ** rng.uniform(19.01, 28, 4 * n)).astype(np.int64)), n)
    else:
        raise ValueError(cls)
    swap = rng.random(n) < 0.5
    return np.where(swap[:, None], np.stack([other, hard], 1), np.stack([hard, other], 1))


# ---- image on a rect -----------------------------------------------------------------------------------
IMAGE_CLASSES = ("uniform", "texel_edge", "rect_edge")


def _image_free(rng, cls, n):
    a0, a1, b0, b1 = IMAGE_RECT
    if cls == "uniform":
        return np.stack([rng.uniform(a0, a1, n), rng.uniform(b0, b1, n)], 1)
    if cls == "texel_edge":                   # u w and v h exact integers in real numbers, and 1 ulp to each side
        x = _ulps(a0 + rng.integers(0, IMG_W + 1, n) * ((a1 - a0) / IMG_W), rng.integers(-1, 2, n))
        y = _ulps(b0 + rng.integers(0, IMG_H + 1, n) * ((b1 - b0) / IMG_H), rng.integers(-1, 2, n))
        return np.stack([np.clip(x, a0, a1), np.clip(y, b0, b1)], 1)
    if cls == "rect_edge":                    # u = 0, u = 1, v = 0, v = 1 and the corners
        x = rng.choice([a0, a1, np.nextafter(a1, a0), np.nextafter(a0, a1)], n)
        y = rng.choice([b0, b1, np.nextafter(b1, b0), np.nextafter(b0, b1)], n)
        free = rng.random(n)
        return np.stack([np.where(free < 0.3, rng.uniform(a0, a1, n), x), np.where(free > 0.7, rng.uniform(b0, b1, n), y)], 1)
    raise ValueError(cls)


# ---- a plane world's points and rays -------------------------------------------------------------------
PlaneSet = namedtuple("PlaneSet", "tex axis classes pts cls rays pinned")
_plane_sets = {}


def plane_classes(tex):
    return CHECKER_CLASSES if tex == "checker" else IMAGE_CLASSES if tex == "image" else NOISE_CLASSES


def plane_set(tex, axis):
    """The points of one plane world (pts, their class cls, whether the reference pins them) and the
    rays that land on them."""
    if (tex, axis) in _plane_sets:
        return _plane_sets[tex, axis]
    classes = plane_classes(tex)
    ka, free = PLANE_AXIS[axis], FREE[axis]
    z_col = free.index(2) if 2 in free else None
    pts, cls = [], []
    for ci, name in enumerate(classes):
        rng = _rng(PLANE_TEXTURES.index(tex), axis, ci)
        n = PER_CLASS if tex != "checker" else 2 * PER_CLASS
        if tex == "checker":
            f = _checker_free(rng, name, n)
        elif tex == "image":
            f = _image_free(rng, name, n)
        else:
            f = _noise_free(rng, name, n, z_col)
        p = np.empty((n, 3))
        p[:, free[0]], p[:, free[1]] = f[:, 0], f[:, 1]
        # the plane constant: pairs of rows share it (the period class's pairs stay in one plane)
        p[:, ka] = np.asarray(K)[rng.integers(0, len(K), (n + 1) // 2).repeat(2)[:n]]
        pts.append(p)
        cls.append(np.full(n, ci))
    pts, cls = np.concatenate(pts), np.concatenate(cls)
    rays = np.zeros(len(pts), dtype=RAY)
    rays["o"] = pts
    rays["o"][:, ka] = pts[:, ka] - 1.0
    assert all(Fraction(float(k)) - 1 == Fraction(float(k) - 1.0) for k in K)       # k - 1 is exact
    rays["d"][:, ka] = 1.0
    rays["t_min"], rays["t_max"] = 0.75, 1.25
    rays["key_pixel"] = np.arange(len(pts))
    pinned = cls != classes.index("unpinned") if "unpinned" in classes else np.ones(len(pts), dtype=bool)
    s = PlaneSet(tex, axis, classes, pts, cls, rays, pinned)
    if tex not in ("checker", "image"):
        big = np.abs(pts[pinned]).max()
        assert big < COORD_LIMIT - 0.5 and np.abs(NOISE_SCALES[tex] * pts[pinned][:, 2]).max() < SIN_DOMAIN, (tex, axis)
    if tex == "checker":
        assert np.abs(10.0 * pts[pinned]).max() <= SIN_DOMAIN
    _plane_sets[tex, axis] = s
    return s


# ---- carrier worlds ---------------------------------------------------------------------------------------
# what a material's record carries: (texture kind, how u and v arise, geometry)
Carrier = namedtuple("Carrier", "name tex uv geom")
CarrierSet = namedtuple("CarrierSet", "rays derived carriers")     # derived: rays whose record is derived by hand
METAL = (0.8, 0.6, 0.3)
NOISE_CARRIER_SCALE = 4.0


def _aimed(rng, centre, reach, size, n, time=None):
    """n rays from a shell of radius `reach` around `centre` towards points within `size` of it;
    directions are not normalised (length 0.5 to 2)."""
    v = rng.normal(size=(n, 3))
    o = centre + reach * v / np.linalg.norm(v, axis=1, keepdims=True)
    w = rng.normal(size=(n, 3))
    target = centre + size * rng.random((n, 1)) ** (1 / 3) * w / np.linalg.norm(w, axis=1, keepdims=True)
    d = target - o
    rays = np.zeros(n, dtype=RAY)
    rays["o"], rays["d"] = o, d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))
    rays["time"] = 0.0 if time is None else time
    rays["t_min"], rays["t_max"] = 0.001, np.inf
    return rays


def _axis_ray(o, d, time=0.0):
    r = np.zeros(1, dtype=RAY)
    r["o"], r["d"], r["time"], r["t_min"], r["t_max"] = o, d, time, 0.001, np.inf
    return r


def _finish(parts):
    rays = np.concatenate([p for p, _ in parts])
    rays["key_pixel"] = np.arange(len(rays))
    rays["key_sample"] = np.arange(len(rays)) % 7
    return rays, np.concatenate([np.full(len(p), flag) for p, flag in parts])


def spheres_world(tw):
    """Spheres only (the final-scene variant holds it). Material handle -> carrier:
      1 an image on a sphere of radius 2 at the origin (poles and seam land exactly, below);
      2 the image as a DiffuseLight on a sphere of radius -1.5 (the outward normal (p - c) / r points inward);
      3 the image on a moving sphere, centre (-10, 0, 0) at time 0 and (-10, 1, 0.5) at time 1;
      4 noise(4) and 5 the checker on spheres: p is the record's; 6 Metal: its albedo; 7 Dielectric: ones."""
    img = tw.image(image())
    c = {}
    c[tw.lambertian(img)] = Carrier("sphere", "image", "sphere", ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.0, 1.0, 2.0))
    c[tw.diffuse_light(img)] = Carrier("negative_radius", "image", "sphere", ((10.0, 0.0, 0.0), (10.0, 0.0, 0.0), 0.0, 1.0, -1.5))
    c[tw.lambertian(img)] = Carrier("moving", "image", "sphere", ((-10.0, 0.0, 0.0), (-10.0, 1.0, 0.5), 0.0, 1.0, 1.25))
    c[tw.lambertian(tw.noise(NOISE_CARRIER_SCALE))] = Carrier("noise_sphere", "noise", None, 0)
    c[tw.lambertian(tw.checker(EVEN, ODD))] = Carrier("checker_sphere", "checker", None, None)
    c[tw.metal(METAL, 0.2)] = Carrier("metal", "metal", None, None)
    c[tw.dielectric(1.5)] = Carrier("dielectric", "ones", None, None)
    m = sorted(c)
    assert m == list(range(1, 8)), m
    tw.push(tw.sphere(m[0], (0.0, 0.0, 0.0), 2.0))
    tw.push(tw.sphere(m[1], (10.0, 0.0, 0.0), -1.5))
    tw.push(tw.moving_sphere(m[2], (-10.0, 0.0, 0.0), (-10.0, 1.0, 0.5), 0.0, 1.0, 1.25))
    tw.push(tw.sphere(m[3], (0.0, 10.0, 0.0), 1.5))
    tw.push(tw.sphere(m[4], (0.0, -10.0, 0.0), 1.5))
    tw.push(tw.sphere(m[5], (0.0, 0.0, 10.0), 1.0))
    tw.push(tw.sphere(m[6], (0.0, 0.0, -10.0), 1.0))
    return c


# Records derived by hand from IEEE 754 and math.rs:288-300, for the 7 x 5 image: (origin, direction) -> (i, j).
# Sphere of radius 2 at the origin. Down the y axis: p = (0, 2, 0), normal (+0, 1, +0): phi = atan2(-0, +0) + pi = pi,
# u = 0.5, i = int(3.5) = 3; theta = acos(-1) = pi, v = 1, 1 - v = 0, j = 0. Up it: normal (+0, -1, +0): u = 0.5, v = 0,
# j = int(5) clamped to 4. Along +x from z = +-1e-300: p = (-2, 0, z): atan2(-z, -1) is -pi for z > 0 and +pi for z < 0
# (rounded: the tiny quotient vanishes), so phi = 0, u = 0, i = 0, or phi = 2 pi, u = 1, i = int(7) clamped to 6; the
# real-number u is 0+ or 1-: the same texels; y = 0 gives v = 0.5, j = int(2.5) = 2.
# Sphere of radius -1.5 at (10, 0, 0). Down the y axis: p = (10, 1.5, 0), normal (0 / -1.5, 1.5 / -1.5, 0 / -1.5) =
# (-0, -1, -0): atan2(+0, -0) = pi, phi = 2 pi, u = 1, i = 6; theta = acos(1) = 0, v = 0, j = 4. Up it: normal
# (-0, 1, -0): u = 1, i = 6; v = 1, j = 0.
DERIVED_SPHERE_RAYS = [
    (((0.0, 5.0, 0.0), (0.0, -1.0, 0.0)), (3, 0)),
    (((0.0, -5.0, 0.0), (0.0, 1.0, 0.0)), (3, 4)),
    (((-5.0, 0.0, 1e-300), (1.0, 0.0, 0.0)), (0, 2)),
    (((-5.0, 0.0, -1e-300), (1.0, 0.0, 0.0)), (6, 2)),
    (((10.0, 5.0, 0.0), (0.0, -1.0, 0.0)), (6, 4)),
    (((10.0, -5.0, 0.0), (0.0, 1.0, 0.0)), (6, 0)),
]


def spheres_set():
    rng = _rng(100)
    parts = [(_axis_ray(o, d), True) for (o, d), _ in DERIVED_SPHERE_RAYS]
    parts.append((_aimed(rng, np.array([0.0, 0.0, 0.0]), 5.0, 1.9, 60), False))
    # both sides of the seam (x < 0, z = +-1e-3 .. 1e-7: u w stays 5e-8 or more from 0 and 7), rounded p
    seam = _aimed(rng, np.array([0.0, 0.0, 0.0]), 5.0, 0.0, 24)
    seam["o"] = np.stack([np.full(24, -5.0), rng.uniform(-1.5, 1.5, 24), rng.choice([-1.0, 1.0], 24) * 10.0 ** -rng.uniform(3, 7, 24)], 1)
    seam["d"] = (1.0, 0.0, 0.0)
    parts.append((seam, False))
    parts.append((_aimed(rng, np.array([10.0, 0.0, 0.0]), 4.0, 1.4, 40), False))
    for time in (0.0, 1.0, 0.5, None):          # the moving sphere at times 0, 1, and in between
        t = rng.uniform(0, 1, 12) if time is None else np.full(12, time)
        centre = np.array([-10.0, 0.0, 0.0]) + t[:, None] * np.array([0.0, 1.0, 0.5])
        parts.append((_aimed(rng, centre, 3.5, 1.1, 12, t), False))
    for centre, size in (((0.0, 10.0, 0.0), 1.4), ((0.0, -10.0, 0.0), 1.4), ((0.0, 0.0, 10.0), 0.9), ((0.0, 0.0, -10.0), 0.9)):
        parts.append((_aimed(rng, np.array(centre), 4.0, size, 24 if size > 1 else 6), False))
    return _finish(parts)


INSTANCE_RECT = (-1.5, 2.0, -0.75, 1.75, 0.0)       # an XZ rect: x0, x1, z0, z1, k
EXACT_OFFSET = (1.5, -2.25, 0.5)
BOX_MAX = (3.5, 2.5, 1.75)
BOX_ANGLE, BOX_OFFSET = 30.0, (20.0, 0.0, 0.0)
NOISE_RECT_ANGLE, NOISE_RECT_OFFSET = -25.0, (-20.0, 0.0, 0.0)
MEDIUM_BOX_OFFSET = (7.3, -20.0, 0.3)      # no face of the box lies in a plane that an axis-parallel ray here runs in
SHUTTER = ((40.0, 0.0, 0.0), (40.0, 1.0, 0.5), 1.0, 0.0, 1.25)     # centre 0, centre 1, time 0 = 1, time 1 = 0, radius


def nested_world(tw):
    """Instances, media and a (1, 0) shutter (the all-features variant). Material handle -> carrier:
      1 the image on translate(rotate_y(XZ rect, 0), EXACT_OFFSET): a rotation by 0 has sin = 0 and cos = 1, so
        the object-space point is p - offset exactly and u, v are the rect's two f64 quotients of it
        (hittable.rs:232-244, 386-415, 339-351), while p is in world space;
      2 the image on translate(rotate_y(box, 30), .): u, v are the object-space face's, p the world's;
      3 noise(4) on translate(rotate_y(XY rect, -25), .): taken at the world-space p;
      4 the image as an isotropic phase function in a sphere: hittable.rs:452-462 leaves u = v = 0, so the
        texel is (0, h - 1) wherever the medium is hit;
      5 noise(4) (its own tables) and 6 the checker as phase functions: taken at the record's p = ray.at(t);
      7 the image on a moving sphere whose shutter is (1, 0): its centre at `time` is
        c0 + ((time - 1) / (0 - 1)) (c1 - c0) (hittable.rs:556-558);
      8 a white boundary material that no record carries."""
    img = tw.image(image())
    c = {}
    c[tw.lambertian(img)] = Carrier("exact_instance", "image", "rect_exact", None)
    c[tw.diffuse_light(img)] = Carrier("instanced_box", "image", "box", None)
    c[tw.lambertian(tw.noise(NOISE_CARRIER_SCALE))] = Carrier("instanced_noise", "noise", None, 0)
    c[tw.isotropic(img)] = Carrier("medium_image", "image", "zero", None)
    c[tw.isotropic(tw.noise(NOISE_CARRIER_SCALE))] = Carrier("medium_noise", "noise", None, 1)
    c[tw.isotropic(tw.checker(EVEN, ODD))] = Carrier("medium_checker", "checker", None, None)
    c[tw.lambertian(img)] = Carrier("shutter", "image", "sphere", SHUTTER)
    white = tw.lambertian(tw.solid(0.73, 0.73, 0.73))
    assert sorted(c) == list(range(1, 8)) and white == 8
    x0, x1, z0, z1, k = INSTANCE_RECT
    tw.push(tw.translate(tw.rotate_y(tw.xz_rect(1, x0, x1, z0, z1, k), 0.0), EXACT_OFFSET))
    tw.push(tw.translate(tw.rotate_y(tw.box((0.0, 0.0, 0.0), BOX_MAX, 2), BOX_ANGLE), BOX_OFFSET))
    tw.push(tw.translate(tw.rotate_y(tw.xy_rect(3, -2.0, 2.0, -2.0, 2.0, 0.5), NOISE_RECT_ANGLE), NOISE_RECT_OFFSET))
    tw.push(tw.constant_medium(tw.sphere(white, (0.0, 20.0, 0.0), 2.0), 2.0, 4))
    tw.push(tw.constant_medium(tw.translate(tw.box((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), white), MEDIUM_BOX_OFFSET), 2.0, 5))
    tw.push(tw.constant_medium(tw.sphere(white, (0.0, 40.0, 0.0), 2.0), 2.0, 6))
    tw.push(tw.moving_sphere(7, *SHUTTER))
    return c


def nested_set():
    rng = _rng(200)
    parts = []
    # the exact instance: rays straight down onto points of the rect, from one unit above it: t = 1
    a0, a1, b0, b1 = IMAGE_RECT
    n = 40
    fx = np.concatenate([_image_free(rng, "uniform", 16), _image_free(rng, "texel_edge", 12), _image_free(rng, "rect_edge", 12)])
    # object-space points on a 2^-20 grid inside the rect, so that adding the offset is exact
    fx = np.clip(np.round(fx * 2.0 ** 20) / 2.0 ** 20, (a0, b0), (a1, b1))
    down = np.zeros(n, dtype=RAY)
    down["o"] = np.stack([fx[:, 0] + EXACT_OFFSET[0], np.full(n, EXACT_OFFSET[1] + 1.0), fx[:, 1] + EXACT_OFFSET[2]], 1)
    down["d"], down["t_min"], down["t_max"] = (0.0, -1.0, 0.0), 0.001, np.inf
    parts.append((down, True))
    parts.append((_aimed(rng, np.array([21.5, 1.2, 0.0]), 6.0, 1.0, 50), False))
    parts.append((_aimed(rng, np.array(NOISE_RECT_OFFSET), 5.0, 1.5, 40), False))
    for centre in ((0.0, 20.0, 0.0), MEDIUM_BOX_OFFSET, (0.0, 40.0, 0.0)):
        parts.append((_aimed(rng, np.array(centre), 5.0, 0.9, 40), False))
    for time in (0.0, 1.0, 0.5, None):
        t = rng.uniform(0, 1, 10) if time is None else np.full(10, time)
        c0, c1 = np.array(SHUTTER[0]), np.array(SHUTTER[1])
        centre = c0 + ((t - 1.0) / (0.0 - 1.0))[:, None] * (c1 - c0)
        parts.append((_aimed(rng, centre, 3.5, 1.1, 10, t), False))
    return _finish(parts)


def plain_world(tw):
    """Spheres with a checker, Metal and Dielectric only: the one world the spheres variant holds, whose
    tex_value knows the checker and solid colours alone. 1 the checker (p is the record's), 2 Metal, 3 Dielectric."""
    c = {tw.lambertian(tw.checker(EVEN, ODD)): Carrier("checker_sphere", "checker", None, None),
         tw.metal(METAL, 0.2): Carrier("metal", "metal", None, None),
         tw.dielectric(1.5): Carrier("dielectric", "ones", None, None)}
    assert sorted(c) == [1, 2, 3]
    tw.push(tw.sphere(1, (0.0, 0.0, 0.0), 2.0))
    tw.push(tw.sphere(2, (10.0, 0.0, 0.0), 1.0))
    tw.push(tw.sphere(3, (-10.0, 0.0, 0.0), -1.0))
    return c


def plain_set():
    rng = _rng(400)
    return _finish([(_aimed(rng, np.array([0.0, 0.0, 0.0]), 5.0, 1.9, 96), False),
                    (_aimed(rng, np.array([10.0, 0.0, 0.0]), 4.0, 0.9, 8), False),
                    (_aimed(rng, np.array([-10.0, 0.0, 0.0]), 4.0, 0.9, 8), False)])


CARRIER_WORLDS = {"plain": (plain_world, plain_set), "spheres": (spheres_world, spheres_set), "nested": (nested_world, nested_set)}


# ---- hard points of the shared transcendentals (include/rt/rt_numerics.h) ----------------------------------
K_LAST = 2 ** 20 - 1        # the last multiple of pi / 2 below the sine's claimed domain |x| < 2^20 pi / 2
_hard = {}


def hard_trig_points():
    """The doubles within +-3 ulp of k pi / 2 for 20,000 k spread over the whole claimed domain (uniform
    in k, every k up to 64, the last hundred), both signs, and |x| = 65536 +- 8 ulp (rt_sin_sign's switch)."""
    if "trig" not in _hard:
        rng = _rng(300)
        k = np.unique(np.concatenate([np.arange(1, 65), np.arange(K_LAST - 99, K_LAST + 1),
                                      rng.integers(65, K_LAST - 99, 19900)]))[:20000]
        near = np.array([float(int(v) * PI / 2) for v in k])
        x = np.concatenate([_ulps(near, n) for n in range(-3, 4)])
        x = x[x < SIN_DOMAIN] * rng.choice([-1.0, 1.0], int((x < SIN_DOMAIN).sum()))
        edge = _ulps(np.full(17, 65536.0), np.arange(-8, 9))
        _hard["trig"] = np.concatenate([x, edge, -edge])
    return _hard["trig"]


def beyond_trig_points(n=2000, top=3.2e7):
    """Doubles within +-3 ulp of m pi for |x| from the end of the claimed domain up to `top`, ascending in |x|."""
    rng = _rng(301)
    m = np.unique(np.round(2.0 ** rng.uniform(19.0, np.log2(top / np.pi), n)).astype(np.int64))
    near = np.array([float(int(v) * PI) for v in m])
    x = np.stack([_ulps(near, j) for j in range(-3, 4)], 1).reshape(-1)
    return x[x >= SIN_DOMAIN]


def hard_atan2_points():
    """(y, x) on the axes and at +-0 in both arguments."""
    z = [0.0, -0.0]
    v = [1.0, -1.0, 5e-324, -5e-324, 1e300, -1e300, 2.5, -0.3]
    pairs = [(a, b) for a in z for b in z] + [(a, b) for a in z for b in v] + [(a, b) for a in v for b in z]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])


def hard_acos_points():
    one = np.array([1.0, 1.0 - 2.0 ** -53, 1.0 - 2.0 ** -52, 1.0 - 2.0 ** -30, 0.5, np.nextafter(0.5, 0), np.nextafter(0.5, 1)])
    return np.concatenate([one, -one, [0.0, -0.0, 2.0 ** -60]])


def hard_log_points():
    """Next to 1: 1 +- j ulp and 1 +- 2^-j, and the first mantissa break sqrt(2) / 2 of the reduction."""
    j = np.arange(1, 53)
    return np.concatenate([_ulps(np.ones(16), np.arange(1, 17)), _ulps(np.ones(16), -np.arange(1, 17)), 1.0 + 2.0 ** -j, 1.0 - 2.0 ** -j,
                           _ulps(np.full(9, np.sqrt(0.5)), np.arange(-4, 5)), _ulps(np.full(9, np.sqrt(2.0)), np.arange(-4, 5))])
