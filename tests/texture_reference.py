"""An independent evaluation of the reference's textures (perlin.rs:32-108, texture.rs:30-75) and of
sphere_uv (math.rs:288-300): no HIP and no oracle, real-number formulas on the f64 inputs taken
exactly. tests/test_texture_reference.py holds oracle/oracle.c to it on the CPU, and
tests/test_gpu_textures.py the kernels, through the fixture tests/golden/texture_expected.npz.

Arithmetic. A point's coordinates, a noise texture's scale and the table entries are doubles; they
enter as `fractions.Fraction`, so floor, the two Hermite smoothings, the eight corner terms, the
seven doublings and the sum are exact rationals. Only the last step, the sine, is not rational:
mpmath evaluates it (and acos / atan2 for sphere_uv) at PREC bits, and the result is rounded to a
double once. The checker needs the sign of sin(a) for a double a != 0, which is never zero (pi is
irrational) and which PREC bits decide for every |a| the tests use (the nearest a double below 2^31
comes to a multiple of pi is far above 2^-100).

The noise bar. 2^-53 (4096 + 4 |scale z|) (tests/texture_points.py's judge applies it) bounds
|f64 evaluation - this one| for any evaluation that does the reference's operations in f64 in the
reference's order, with or without contracted multiply-adds (which only remove roundings). With e = 2^-53,
every f64 operation contributing a relative error of at most e:
  u = p - floor(p) is exact (|p| < 2^52). us = u u (3 - 2u): three roundings, relative 3e.
  uu = us us (3 - 2 us): the inherited 3e grows by d ln uu / d ln us = 6 (1 - us) / (3 - 2 us) <= 2, plus
  three roundings: absolute 9e; 1 - uu one more: each of the six weight factors is off by d <= 10e.
  A corner's weight W = Wx Wy Wz. Summed over the eight corners, the factor errors give
  sum |dW| <= 3 * 2d + 2e = 62e (the two factors of an axis sum to 1, so sum_corners dx Wy Wz = (dx0 + dx1)).
  The dot product c . (us - i, vs - j, ws - k), |c| = 1: components off by 4e each, three products
  and two sums: absolute 16e, and |dot| <= sqrt 3.
  noise = sum W dot: sqrt 3 * 62e + 16e (sum W = 1) + 2e (the products) + 14e (eight sums of
  partial sums <= sqrt 3) < 140e.
  turb: the octave weights are powers of two and sum to < 2: 280e, and seven sums of |accum| <= 2 sqrt 3:
  25e: < 305e. Times 10 and that product's rounding: < 3085e + 35e.
  The argument scale z + 10 turb: the product scale z rounds by e |scale z|, the sum by
  e (|scale z| + 35): the argument is off by < 3160e + 2e |scale z|. The sine has slope <= 1 and the
  header's 2 ulp (<= 2e for |sin| <= 1); 1 + sin rounds by 2e; times 0.5 is exact: the value is off by
  < 1582e + e |scale z|, and the fixture's own rounding to a double adds e / 2.
So the bar of 4096e + 4e |scale z| holds with a factor of 2.5 to spare; the CPU test asserts that
the oracle's measured maximum stays under a quarter of it.
"""
import math
from fractions import Fraction

import mpmath
import numpy as np

PREC = 400
SQRT3 = math.sqrt(3.0)


class Tables:
    """ranvec[256][3] and perm[3][256] (x, y, z) of one Perlin instance, as exact rationals / ints."""

    def __init__(self, ranvec, perm):
        ranvec = np.asarray(ranvec, dtype=np.float64).reshape(256, 3)
        perm = np.asarray(perm).reshape(3, 256)
        self.ranvec = [tuple(Fraction(float(c)) for c in row) for row in ranvec]
        self.perm = [[int(v) for v in row] for row in perm]


def _hermite(t):
    return t * t * (3 - 2 * t)


def _frac3(p):
    """Doubles taken exactly (a Fraction passes as it is: the self-checks step off the doubles)."""
    return [c if isinstance(c, Fraction) else Fraction(float(c)) for c in p]


def _noise(tables, p):
    """perlin.rs:32-94 on a point of three Fractions."""
    cell = [math.floor(c) for c in p]                      # exact: Fraction.__floor__
    once = [_hermite(c - f) for c, f in zip(p, cell)]      # :41-43, the first smoothing
    twice = [_hermite(t) for t in once]                    # :71-73, the second
    total = Fraction(0)
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                d = (di, dj, dk)
                # :54-61; Python's & on a negative int is two's complement, as i32's
                idx = (tables.perm[0][(cell[0] + di) & 255] ^ tables.perm[1][(cell[1] + dj) & 255] ^
                       tables.perm[2][(cell[2] + dk) & 255]) & 255
                c = tables.ranvec[idx]
                weight = Fraction(1)
                for a in range(3):
                    weight *= twice[a] if d[a] else 1 - twice[a]
                total += weight * sum(c[a] * (once[a] - d[a]) for a in range(3))
    return total


def noise(tables, p):
    return _noise(tables, _frac3(p))


def turb(tables, p, depth=7):
    """perlin.rs:96-108: sum of 2^-i noise(2^i p), then abs. Exact."""
    q = _frac3(p)
    total = Fraction(0)
    for i in range(depth):
        total += Fraction(1, 2 ** i) * _noise(tables, [c * 2 ** i for c in q])
    return abs(total)


def _mpf(fr):
    return mpmath.mpf(fr.numerator) / mpmath.mpf(fr.denominator)


def noise_value(tables, scale, p):
    """texture.rs:43-45: 0.5 (1 + sin(scale z + 10 turb(p, 7))), rounded to a double once."""
    arg = Fraction(float(scale)) * Fraction(float(p[2])) + 10 * turb(tables, p, 7)
    with mpmath.workprec(PREC + 64):
        return float((1 + mpmath.sin(_mpf(arg))) / 2)


def sin_sign(a):
    """The sign of sin(a) for a double a: 0 only at a = 0."""
    a = float(a)
    if a == 0.0:
        return 0
    with mpmath.workprec(PREC):
        s = mpmath.sin(mpmath.mpf(a))
        assert abs(s) > mpmath.mpf(2) ** -(PREC // 2), a
        return 1 if s > 0 else -1


def checker_odd(p):
    """texture.rs:35-41: sin(10 x) sin(10 y) sin(10 z) < 0, the three products 10 p_i rounded as IEEE
    rounds them. A zero factor makes the product zero, which is not < 0."""
    signs = [sin_sign(np.float64(10.0) * np.float64(c)) for c in p]
    return signs[0] * signs[1] * signs[2] < 0


def image_texel(w, h, u, v):
    """texture.rs:46-63 on doubles u, v, with the reference's own f64 operations (a clamp, one
    subtraction, two products, two truncations), which numpy's float64 performs identically: (i, j)."""
    u, v = np.float64(u), np.float64(v)
    uu = min(max(u, np.float64(0.0)), np.float64(1.0))
    vv = np.float64(1.0) - min(max(v, np.float64(0.0)), np.float64(1.0))
    i, j = int(uu * np.float64(w)), int(vv * np.float64(h))
    return min(i, w - 1), min(j, h - 1)


def rect_uv(x, y, a0, a1, b0, b1):
    """hittable.rs:323-376: the two f64 quotients of a rect's record."""
    x, y, a0, a1, b0, b1 = (np.float64(t) for t in (x, y, a0, a1, b0, b1))
    return (x - a0) / (a1 - a0), (y - b0) / (b1 - b0)


def _atan2(y, x):
    """atan2 of two doubles in mpmath, with IEEE 754's rules where y is a signed zero (mpmath has no
    -0): atan2(+-0, x > 0 or +0) = +-0, atan2(+-0, x < 0 or -0) = +-pi."""
    if y == 0.0:
        neg_x = x < 0.0 or (x == 0.0 and math.copysign(1.0, x) < 0.0)
        if not neg_x:
            return mpmath.mpf(0)
        return -mpmath.pi if math.copysign(1.0, y) < 0.0 else +mpmath.pi
    return mpmath.atan2(mpmath.mpf(y), mpmath.mpf(x))


def sphere_texel(w, h, p, center, radius):
    """texture.rs:46-63 over math.rs:288-300 of the outward normal (p - center) / radius (radius
    signed: hittable.rs:276-279), in mpmath: ((i, j), distance of u w and of (1 - v) h from the
    nearest integer). The normal's three components are formed as the reference forms them (an f64
    difference and an f64 quotient), since their signs of zero decide atan2 at the poles."""
    n = [(np.float64(a) - np.float64(c)) / np.float64(radius) for a, c in zip(p, center)]
    with mpmath.workprec(PREC):
        # a unit vector up to rounding: acos of a |y| barely over 1 would be NaN in the reference too
        ny = max(-1.0, min(1.0, float(n[1])))
        theta = mpmath.acos(-mpmath.mpf(ny))
        phi = _atan2(-float(n[2]), float(n[0])) + mpmath.pi
        u = phi / (2 * mpmath.pi)
        v = theta / mpmath.pi
        uw = min(max(u, 0), 1) * w
        vh = (1 - min(max(v, 0), 1)) * h
        i, j = min(int(mpmath.floor(uw)), w - 1), min(int(mpmath.floor(vh)), h - 1)
        return (i, j), (float(abs(uw - mpmath.nint(uw))), float(abs(vh - mpmath.nint(vh))))


def truth(f, *args, prec=240):
    """f (an mpmath function) of the doubles in args at `prec` bits, as two doubles per value: hi, the
    value rounded, and lo = value - hi rounded: hi + lo carries the truth to about 2^-106 relative."""
    n = len(args[0])
    hi, lo = np.empty(n), np.empty(n)
    with mpmath.workprec(prec):
        for i in range(n):
            v = f(*[mpmath.mpf(float(a[i])) for a in args])
            hi[i] = float(v)
            lo[i] = float(v - mpmath.mpf(hi[i]))
    return hi, lo


def ulp_error(got, hi, lo):
    """|got - (hi + lo)| in units of the truth's last place; got - hi is exact for values this close."""
    got = np.asarray(got, dtype=np.float64)
    return np.abs((got - hi) - lo) / np.spacing(np.abs(hi))
