"""Worlds whose pixel depends on the draw and whose expectation has a closed form, and their statistics.

HIP-free, numpy only, in the manner of tests/path_free_worlds.py (whose Spec, camera24, BG and
lattice_j are reused). On the path-independent worlds a wrong lobe, free path, Schlick probability
or shutter time changes no pixel. Here every sample is one of two exact values, bright or dark, so
a pixel carries an integer count j of bright samples (the lattice of path_free_worlds.py), and j is
Binomial(spp, p) with p known in f64 from a formula that uses none of the renderer's code:

- absorb: a constant medium of density rho with a black isotropic phase. A sample is bg
  (transmitted) or 0; p = exp(-rho L), L the chord through the boundary (Beer-Lambert;
  hittable.rs:417-473 draws -1/rho log(u) against it). Boundaries: a sphere, a box, a
  translate(rotate_y(box)).
- schlick: a glass shell around a black core. A sample is bg (reflected or missed) or 0 (refracted:
  the refracted ray's impact parameter is at most r/ir < the core's radius, so it meets the core);
  p = r0 + (1 - r0)(1 - cos)^5 (material.rs:62-94).
- lobe: a Lambertian floor of albedo a under a black rectangle. A sample is a bg (the bounce
  escaped) or 0 (it met the blocker); the bounce normal + unit vector (material.rs:36-48) is cosine
  distributed, so p = 1 - F, F the view factor from a surface element to a parallel rectangle.
- shutter: a black moving sphere. A sample is 0 while the sphere covers the ray, else bg; p is one
  minus the share of the shutter interval in which the centre (hittable.rs:556-558) is within r of
  the ray, the root interval of a quadratic in the time (camera.rs:58-66 draws it uniformly).

Oracle-referenced worlds (names oracle-ref/...) are two-valued in the same way but have no closed
form here: a fuzzy mirror floor under the blocker, and the moving sphere as an emitter through a
finite aperture. Their p is the oracle's pooled count over REF_SEEDS seeds and the pool's own
variance enters every z; they compare a kernel with the oracle, they are not closed-form evidence.

The pixel ray is llc + s hor + t ver - origin with s = (x + xi)/(W - 1), t = (y + xi)/(H - 1)
(main.rs:517-518); p(x, y) is the mean of the closed form over a K x K midpoint grid in the pixel,
K = 16, with the cells a silhouette crosses refined (pixel_p; tests/test_transport_worlds.py
asserts that K = 32 moves no p by more than 1e-4).

Bars (derived, not measured): every |z| <= Z_MAX = 5 on the total count, on up to ten bins of
pixels ordered by p, and on chi^2. Across the ~500 statistics of the suite the chance of a false
alarm is ~500 * 5.7e-7 = 3e-4, while a 1 % bias in a draw moves the total by >= 15 sigma at SPP.
The render seed is 1. Lattice tolerance on j: the f32 rounding bound times 32, as in
tests/test_gpu_f32_exact.py: a sample is n roundings of 2^-24 relative (bg: 1, a bg: 3) and the
same value repeats, so |dj| <= n 2^-24 spp / (1 - max dark/bright); no pixel may leave the lattice.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from tests import path_free_worlds as pf
from tests.path_free_worlds import ALL, BG, MEDIA, RECTINST

W, H = 32, 24
K = 16                 # sub-pixel midpoint grid of the closed forms
SPP = 16384            # 12.6 M samples per world; below 4096 a 0.5 % chord or a 2 % Schlick fault is under 5 sigma
PARITY_SPP = 8         # the f64 kernel against the oracle, path for path
Z_MAX = 5.0
REF_SEEDS = tuple(range(101, 109))     # oracle-referenced worlds: 8 x SPP samples, variance 1/8 of one run's
ALBEDO = (0.5, 0.4, 0.3)
EMIT = (0.35, 0.32, 0.3)               # the emitter sphere: <= bg / 2 on every channel

assert SPP & (SPP - 1) == 0 and SPP >= 4096


@dataclass
class TSpec(pf.Spec):
    """A two-valued world: a sample is `bright` or `dark`; prob(o, d) is the closed-form chance of
    bright for rays o + s d (None: oracle-referenced); rounds is the number of f32 roundings in a
    sample value."""
    W: int = W
    H: int = H
    spp: int = PARITY_SPP
    bright: tuple = BG
    dark: tuple = (0.0, 0.0, 0.0)
    rounds: int = 1
    prob: Optional[Callable] = None
    aperture: float = 0.0
    time0: float = 0.0
    time1: float = 1.0

    def cam24(self):
        return pf.camera24(self.look_from, self.look_at, self.vfov, self.W / self.H, self.vup, self.aperture, 10.0,
                           self.time0, self.time1)

    @property
    def j_tol(self):
        ratio = max(d / b for d, b in zip(self.dark, self.bright))
        return 32.0 * self.rounds * 2.0 ** -24 * SPP / (1.0 - ratio)


# ---- rays and closed forms --------------------------------------------------------------------

REFINE, LEVELS, BILINEAR_TOL = 4, 3, 2e-4


def _midpoints(f, x0, y0, h, levels):
    """The midpoint value of f over the cells [x0, x0 + h] x [y0, y0 + h]; a cell whose centre is
    more than BILINEAR_TOL off the mean of its corners (a silhouette, or the square-root kink
    beside one, crosses it: a smooth cell is bilinear to ~h^2 f''/4) is the mean of its
    REFINE x REFINE sub-cells instead, to LEVELS levels."""
    c = f(x0 + 0.5 * h, y0 + 0.5 * h)
    if levels == 0:
        return c
    corners = 0.25 * (f(x0, y0) + f(x0 + h, y0) + f(x0, y0 + h) + f(x0 + h, y0 + h))
    idx = np.nonzero(np.abs(corners - c) > BILINEAR_TOL)[0]
    if idx.size:
        sub = h / REFINE
        off = np.arange(REFINE) * sub
        cx = (x0[idx, None, None] + off[None, None, :] + 0.0 * off[None, :, None]).reshape(-1)
        cy = (y0[idx, None, None] + off[None, :, None] + 0.0 * off[None, None, :]).reshape(-1)
        c[idx] = _midpoints(f, cx, cy, sub, levels - 1).reshape(-1, REFINE * REFINE).mean(axis=1)
    return c


def pixel_p(spec, k=K):
    """The closed-form chance of a bright sample per pixel, (H, W): the mean over the pixel's
    k x k midpoint grid, cells on a silhouette refined (_midpoints; the plain grid leaves an edge
    pixel's p ~1e-2 off where p jumps, against the 1e-4 the statistics need)."""
    cam = spec.cam24()
    o, llc, hor, ver = cam[0:3], cam[3:6], cam[6:9], cam[9:12]

    def f(x, y):     # the pixel ray, main.rs:517-518 and camera.rs:58-66 at aperture 0
        d = (llc - o) + (x / (spec.W - 1.0))[:, None] * hor + (y / (spec.H - 1.0))[:, None] * ver
        return spec.prob(o, d)

    g = np.arange(k) / k
    y0 = (np.arange(spec.H)[:, None, None, None] + g[None, None, :, None] + np.zeros((1, spec.W, 1, k))).reshape(-1)
    x0 = (np.arange(spec.W)[None, :, None, None] + g[None, None, None, :] + np.zeros((spec.H, 1, k, 1))).reshape(-1)
    return _midpoints(f, x0, y0, 1.0 / k, LEVELS).reshape(spec.H, spec.W, k * k).mean(axis=-1)


def ray_sphere(o, d, centre, r):
    """(a, hb, disc) of |o + s d - centre|^2 = r^2 in the half-b form: roots (-hb -+ sqrt(disc))/a."""
    oc = o - np.asarray(centre, dtype=np.float64)
    a = np.sum(d * d, axis=-1)
    hb = np.sum(oc * d, axis=-1)
    return a, hb, hb * hb - a * (np.sum(oc * oc, axis=-1) - r * r)


def _norm(d):
    return np.sqrt(np.sum(d * d, axis=-1))


def p_absorb_sphere(rho, centre, r):
    def prob(o, d):
        a, _, disc = ray_sphere(o, d, centre, r)
        return np.exp(-rho * 2.0 * np.sqrt(np.maximum(disc, 0.0)) / np.sqrt(a))     # chord 2 sqrt(disc)/|d|
    return prob


def slab_chord(o, d, mn, mx):
    """Length of the ray o + s d, s >= 0, inside the box [mn, mx]."""
    with np.errstate(divide="ignore"):
        t0, t1 = (np.asarray(mn) - o) / d, (np.asarray(mx) - o) / d
    near, far = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)
    return np.maximum(far - np.maximum(near, 0.0), 0.0) * _norm(d)


def to_instance(o, d, angle, offset):
    """The ray in the frame of translate(rotate_y(child, angle), offset) (hittable.rs:232-244, 386-415)."""
    s, c = np.sin(np.radians(angle)), np.cos(np.radians(angle))
    rot = np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])
    return rot @ (o - np.asarray(offset, dtype=np.float64)), d @ rot.T


def p_absorb_box(rho, mn, mx, angle=None, offset=None):
    def prob(o, d):
        if angle is not None:
            o, d = to_instance(o, d, angle, offset)
        return np.exp(-rho * slab_chord(o, d, mn, mx))
    return prob


def p_schlick(ir, r):
    def prob(o, d):
        a, hb, disc = ray_sphere(o, d, (0.0, 0.0, 0.0), r)
        hit = disc > 0.0
        t = (-hb - np.sqrt(np.maximum(disc, 0.0))) / a
        n = (o + t[..., None] * d) / r
        cos = np.minimum(-np.sum(d * n, axis=-1) / np.sqrt(a), 1.0)
        r0 = ((1.0 - 1.0 / ir) / (1.0 + 1.0 / ir)) ** 2
        return np.where(hit, r0 + (1.0 - r0) * (1.0 - cos) ** 5, 1.0)
    return prob


def _corner(x, y):
    """View factor from a surface element to a parallel rectangle one unit above it with a corner
    over the element and sides x, y (odd in both)."""
    ax, ay = np.sqrt(1.0 + x * x), np.sqrt(1.0 + y * y)
    return (x / ax * np.arctan(y / ax) + y / ay * np.arctan(x / ay)) / (2.0 * np.pi)


def view_factor(px, pz, x0, x1, z0, z1, h):
    """From an upward element at (px, 0, pz) to the rectangle [x0, x1] x [z0, z1] at height h."""
    xa, xb, za, zb = (x0 - px) / h, (x1 - px) / h, (z0 - pz) / h, (z1 - pz) / h
    return _corner(xb, zb) - _corner(xa, zb) - _corner(xb, za) + _corner(xa, za)


BLOCKER = (-1.0, 0.6, -0.8, 1.0, 0.7)      # x0, x1, z0, z1, y


def p_lobe(o, d):
    assert np.all(d[..., 1] < 0.0) and o[1] < BLOCKER[4], "every primary ray must reach the floor"
    t = -o[1] / d[..., 1]
    px, pz = o[0] + t * d[..., 0], o[2] + t * d[..., 2]
    assert np.abs(px).max() < 50.0 and np.abs(pz).max() < 50.0
    x0, x1, z0, z1, h = BLOCKER
    return 1.0 - view_factor(px, pz, x0, x1, z0, z1, h)


MOVER = ((-1.2, -0.2, 0.0), (1.0, 0.5, 0.3), 0.45)     # centre at time 0, at time 1, radius


def p_shutter(time0, time1):
    def prob(o, d):
        c0, c1, r = (np.asarray(x, dtype=np.float64) for x in MOVER)
        u = d / _norm(d)[..., None]

        def perp(v):
            return v - np.sum(v * u, axis=-1)[..., None] * u
        a_, b_ = perp(c0 - o), perp(c1 - c0)            # distance^2 to the ray at time t: |a_ + t b_|^2
        qa, qb, qc = np.sum(b_ * b_, axis=-1), np.sum(a_ * b_, axis=-1), np.sum(a_ * a_, axis=-1) - r * r
        disc = qb * qb - qa * qc
        sq = np.sqrt(np.maximum(disc, 0.0))
        lo, hi = np.maximum((-qb - sq) / qa, time0), np.minimum((-qb + sq) / qa, time1)
        covered = np.where(disc > 0.0, np.maximum(hi - lo, 0.0), 0.0) / (time1 - time0)
        return 1.0 - covered
    return prob


# ---- the worlds -------------------------------------------------------------------------------

def _black(w):
    return w.lambertian(w.solid(0.0, 0.0, 0.0))


def _absorb(rho, boundary):
    def build(w):
        w.push(w.constant_medium(boundary(w, _black(w)), rho, w.isotropic(w.solid(0.0, 0.0, 0.0))))
    return build


ROT_BOX = ((0.0, 0.0, 0.0), (1.6, 1.6, 1.6), 30.0, (-1.1, -0.8, -0.3))


def _blocker(w):
    x0, x1, z0, z1, y = BLOCKER
    w.push(w.xz_rect(_black(w), x0, x1, z0, z1, y))


def _floor_rect(mat):
    def build(w):
        w.push(w.xz_rect(mat(w), -50.0, 50.0, -50.0, 50.0, 0.0))
        _blocker(w)
    return build


def _floor_box(w):
    top = w.box((-50.0, -1.0, -50.0), (50.0, 0.0, 50.0), w.lambertian(w.solid(*ALBEDO)))
    w.push(w.translate(w.rotate_y(top, 20.0), (0.3, 0.0, -0.2)))
    _blocker(w)


def _schlick(ir):
    def build(w):
        w.push(w.sphere(w.dielectric(ir), (0.0, 0.0, 0.0), 1.0))
        w.push(w.sphere(_black(w), (0.0, 0.0, 0.0), 0.9))
    return build


def _mover(mat):
    def build(w):
        c0, c1, r = MOVER
        w.push(w.moving_sphere(mat(w), c0, c1, 0.0, 1.0, r))
    return build


def closed_form_worlds() -> list:
    a_bg = tuple(a * b for a, b in zip(ALBEDO, BG))
    view = dict(look_from=(0.0, 0.3, 4.0), look_at=(0.0, 0.0, 0.0), vfov=36.0, features=MEDIA)
    out = [TSpec(f"absorb-{rho}", _absorb(rho, lambda w, m: w.sphere(m, (0.0, 0.0, 0.0), 1.0)),
                 prob=p_absorb_sphere(rho, (0.0, 0.0, 0.0), 1.0), **view) for rho in (0.05, 0.7, 8.0)]
    out.append(TSpec("absorb-0.7-box", _absorb(0.7, lambda w, m: w.box((-0.8, -0.8, -0.8), (0.8, 0.8, 0.8), m)),
                     prob=p_absorb_box(0.7, (-0.8, -0.8, -0.8), (0.8, 0.8, 0.8)), **view))
    mn, mx, angle, off = ROT_BOX
    out.append(TSpec("absorb-0.7-rotbox",
                     _absorb(0.7, lambda w, m: w.translate(w.rotate_y(w.box(mn, mx, m), angle), off)),
                     prob=p_absorb_box(0.7, mn, mx, angle, off), **view))
    # ragged tiles: 37 x 21 is a multiple of the 8 x 8 tile in neither axis
    out.append(TSpec("absorb-0.7-37x21", out[1].build, prob=out[1].prob, W=37, H=21, **view))
    for ir in (1.5, 2.4):
        out.append(TSpec(f"schlick-{ir}", _schlick(ir), (0.0, 0.3, 3.0), (0.0, 0.0, 0.0), 45.0, prob=p_schlick(ir, 1.0)))
    lobe = dict(look_from=(0.0, 0.5, 1.5), look_at=(0.0, 0.0, 0.3), vfov=30.0, features=RECTINST, bright=a_bg, rounds=3,
                prob=p_lobe)
    out.append(TSpec("lobe", _floor_rect(lambda w: w.lambertian(w.solid(*ALBEDO))), **lobe))
    out.append(TSpec("lobe-rotbox", _floor_box, **lobe))
    out.append(TSpec("shutter", _mover(_black), (0.0, 0.2, 4.0), (0.0, 0.0, 0.0), 36.0, prob=p_shutter(0.0, 1.0)))
    out.append(TSpec("shutter-0.2-0.6", _mover(_black), (0.0, 0.2, 4.0), (0.0, 0.0, 0.0), 36.0, prob=p_shutter(0.2, 0.6),
                     time0=0.2, time1=0.6))
    return out


def oracle_ref_worlds() -> list:
    a_bg = tuple(a * b for a, b in zip(ALBEDO, BG))
    floor = dict(look_from=(0.0, 0.5, 1.5), look_at=(0.0, 0.0, 0.3), vfov=30.0, features=RECTINST, bright=a_bg, rounds=3)
    return [TSpec("oracle-ref/mirror-fuzz0.3", _floor_rect(lambda w: w.metal(ALBEDO, 0.3)), **floor),
            TSpec("oracle-ref/mirror-fuzz1.0", _floor_rect(lambda w: w.metal(ALBEDO, 1.0)), **floor),
            TSpec("oracle-ref/emitter-aperture0.3", _mover(lambda w: w.diffuse_light(w.solid(*EMIT))), (0.0, 0.2, 4.0),
                  (0.0, 0.0, 0.0), 36.0, dark=EMIT, aperture=0.3)]


for _s in closed_form_worlds() + oracle_ref_worlds():
    assert _s.j_tol < 0.1, (_s.name, _s.j_tol)


def texel_image() -> np.ndarray:
    """8 x 4 texels of palette() colours as u8 (15.3 k per 0.06 step: still >= 15/255 apart)."""
    return np.rint(np.array(pf.palette(32)).reshape(4, 8, 3) * 255.0).astype(np.uint8)


def texel_world() -> pf.Spec:
    """One more ID world: a sphere and an xz_rect that emit an 8 x 4 image, so an interior pixel is
    a texel's colour, and the f32 u, v -> texel mapping is held per pixel."""
    s = pf.Spec("id-texels", None, (0.5, 3.0, 6.0), (0.3, 0.6, 0.0), 30.0, W=160, H=100, spp=4, features=ALL, albedo=None)

    def build(w):
        img = texel_image()
        s.owners = [(tuple(c / 255.0), "texel") for c in img.reshape(-1, 3).astype(np.float64)]
        w.push(w.sphere(w.diffuse_light(w.image(img)), (-1.3, 1.0, 0.0), 1.0))
        w.push(w.xz_rect(w.diffuse_light(w.image(img)), 0.0, 2.8, -1.6, 1.6, 0.0))
    s.build = build
    return s


# ---- counts and statistics --------------------------------------------------------------------

def bright_count(img, spec, spp, tol):
    """(ok, j): j the per-pixel count of bright samples, ok where the three channels give that
    one integer in [0, spp] within tol."""
    ratio = np.asarray(spec.dark, dtype=np.float64) / np.asarray(spec.bright, dtype=np.float64)
    ok, dark = pf.lattice_j(img, spec.bright, ratio, spp, tol)
    return ok, spp - dark


def lattice_dev(img, spec, spp):
    """The largest distance of a channel's j from the first channel's integer."""
    ratio = np.asarray(spec.dark, dtype=np.float64) / np.asarray(spec.bright, dtype=np.float64)
    jc = pf.channel_j(img, spec.bright, ratio, spp)
    return float(np.abs(jc - np.rint(jc[..., :1])).max())


def variance(p, spp, ref_samples=None):
    """Var(j - spp p) per pixel; with p estimated from ref_samples samples per pixel its own
    variance is added."""
    v = spp * p * (1.0 - p)
    return v if ref_samples is None else v * (1.0 + spp / ref_samples)


def z_total(j, p, spp, ref_samples=None):
    return float((j.sum() - spp * p.sum()) / np.sqrt(variance(p, spp, ref_samples).sum()))


def z_bins(j, p, spp, ref_samples=None, n_bins=10, min_var=100.0):
    """z_total on bins of pixels ordered by p: ten bins of equal pixel count, neighbours merged
    until each bin's variance is at least min_var."""
    order = np.argsort(p, axis=None, kind="stable")
    dev = (j.reshape(-1) - spp * p.reshape(-1))[order]
    var = variance(p, spp, ref_samples).reshape(-1)[order]
    bins = [[float(d.sum()), float(v.sum())] for d, v in zip(np.array_split(dev, n_bins), np.array_split(var, n_bins))]
    merged = []
    for d, v in bins:
        if merged and merged[-1][1] < min_var:
            merged[-1][0] += d
            merged[-1][1] += v
        else:
            merged.append([d, v])
    if len(merged) > 1 and merged[-1][1] < min_var:
        d, v = merged.pop()
        merged[-1][0] += d
        merged[-1][1] += v
    return np.array([d / np.sqrt(v) for d, v in merged if v > 0.0])


def chi2(j, p, spp, ref_samples=None, min_var=25.0):
    """(mean, z, dof): the mean of (j - spp p)^2 / var over the pixels with spp p (1 - p) >= min_var,
    and its z against 1 +- sqrt(2 / dof)."""
    var = variance(p, spp, ref_samples)
    m = spp * p * (1.0 - p) >= min_var
    dof = int(m.sum())
    if dof == 0:
        return 1.0, 0.0, 0
    mean = float(np.mean((j[m] - spp * p[m]) ** 2 / var[m]))
    return mean, float((mean - 1.0) / np.sqrt(2.0 / dof)), dof


def statistics(j, p, spp, ref_samples=None) -> dict:
    zb = z_bins(j, p, spp, ref_samples)
    mean, zc, dof = chi2(j, p, spp, ref_samples)
    return {"z_total": z_total(j, p, spp, ref_samples), "z_bin": float(zb[np.argmax(np.abs(zb))]), "bins": len(zb),
            "chi2": mean, "z_chi2": zc, "dof": dof, "ratio": float(j.sum() / (spp * p.sum()) - 1.0)}


def describe(tag, st) -> str:
    return (f"{tag}: z_total {st['z_total']:+.2f}, worst of {st['bins']} bins {st['z_bin']:+.2f}, chi2/dof {st['chi2']:.3f} "
            f"(z {st['z_chi2']:+.2f}, {st['dof']} px), sum j / (spp sum p) - 1 = {st['ratio']:+.2e}")


def failures(st) -> list:
    return [k for k in ("z_total", "z_bin", "z_chi2") if not abs(st[k]) <= Z_MAX]


def pooled_p(imgs, spec, spp, tol):
    """(p, ref_samples, ok): the pooled bright share of several renders of spp samples each."""
    counts = [bright_count(im, spec, spp, tol) for im in imgs]
    ok = np.all([c[0] for c in counts], axis=0)
    n = len(imgs) * spp
    return np.sum([c[1] for c in counts], axis=0) / n, n, ok
