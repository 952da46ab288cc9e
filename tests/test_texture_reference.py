"""The textures and the math under them, held to an independent evaluation on the CPU.

tests/texture_reference.py restates perlin.rs:32-108, texture.rs:30-75 and math.rs:288-300 as
real-number formulas (exact rationals, mpmath for the sine); it shares nothing with oracle/oracle.c,
csrc/trace_shade.hpp or the product's table builder, which all came from one reading of the
reference. Here the reference is checked against properties that follow from perlin.rs alone, the
product's Perlin tables against what perlin.rs:13-30, 110-129 make, and the oracle's albedo
(OracleWorld.hit) against the reference at every point of tests/texture_points.py; the committed
fixture tests/golden/texture_expected.npz, which tests/test_gpu_textures.py holds the kernels to,
is regenerated and must be equal. The last part holds rt_sin, rt_cos, rt_sin_sign, rt_atan2, rt_acos
and rt_log (include/rt/rt_numerics.h) to mpmath at their hard points, and marks where the sine's
domain ends.

Measured (printed by the tests): the oracle's largest noise error is 0.19 of its bar (1.4e-11 at
|scale z| = 2.5e5, where the rounding of the sine's argument dominates; 8.9e-14, 0.06 of the bar,
at |p| <= 257); checker, image, pole, seam, medium and instance records are equal on all 1,984
points; no sphere- or instance-borne image point is left out (0 of 262, the smallest distance of
u w or v h from an integer 9.0e-8); rt_sin 0.66 ulp, rt_cos 0.50 ulp and every sign right on 139,103
doubles within 3 ulp of k pi / 2 over the whole claimed domain; past it the first wrong sign this
file's set finds is at |x| = 1.678e7 (DESIGN.md section 3 has the denser scan).

Each of five deliberate misreadings of a scratch copy of oracle.c makes this file fail: a single
smoothing, p[target] written in place of the index, a six-octave turb, `<=` in the checker, an
unflipped v (the first three and the last fail both oracle tests, the checker's the plane test).
"""
import ctypes
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from tests import oracle_binding as ob
from tests import texture_points as tp
from tests import texture_reference as tr
from tests.golden import make_texture_fixture as mk


@pytest.fixture(scope="module")
def generated(rt):
    return mk.generate(rt)


@pytest.fixture(scope="module")
def tables(rt):
    """The Perlin instance of the noise4 plane worlds (one per world; the seed and the draws before
    it are the same on the three axes, and so are the tables)."""
    per_axis = [mk.product_tables(rt, lambda w, a=axis: tp.plane_world(w, "noise4", a)) for axis in range(3)]
    assert all(np.array_equal(per_axis[0][1], t[1]) and np.array_equal(per_axis[0][2], t[2]) for t in per_axis)
    return per_axis[0][0][0]


def test_fixture_is_what_the_reference_gives(generated):
    arrays, report = generated
    with np.load(mk.FIXTURE) as committed:
        assert sorted(committed.files) == sorted(arrays)
        for key, want in arrays.items():
            assert committed[key].dtype == want.dtype and np.array_equal(committed[key], want), key
    left_out = sum(report[w]["left_out"] for w in tp.CARRIER_WORLDS)
    judged = sum(report[w]["random_image_points"] for w in tp.CARRIER_WORLDS)
    for w in tp.CARRIER_WORLDS:
        print(w, report[w])
    print(f"sphere- and instance-borne image points left out: {left_out} of {judged}")
    assert left_out <= 0.005 * judged          # the reference alone meets the cap
    # every carrier is reached, and media both scatter and let rays through
    for w in tp.CARRIER_WORLDS:
        assert min(report[w]["per_carrier"].values()) >= 5, report[w]


# ---- the reference against itself: what follows from perlin.rs, not from an implementation -----------------
def test_noise_has_period_256(tables):
    n = 0
    for axis in range(3):
        s = tp.plane_set("noise4", axis)
        rows = np.flatnonzero(s.cls == s.classes.index("period"))
        for a, b in zip(rows[0::2], rows[1::2]):
            d = s.pts[b] - s.pts[a]
            assert sorted(np.abs(d)) == [0.0, 0.0, 256.0], d
            assert tr.turb(tables, s.pts[a]) == tr.turb(tables, s.pts[b])        # exact rationals
            n += 1
    assert n >= 40


def test_noise_is_continuous_across_lattice_planes(tables):
    """Each octave's noise is a polynomial per cell whose gradient is bounded (|d noise / d x| < 16), so
    values 2^-90 to either side of a lattice plane differ by far less than 1e-25 if the cells agree
    on the plane: the corner indices and weights of perlin.rs:51-88 have to line up."""
    rng = np.random.default_rng(3)
    step = Fraction(1, 2 ** 90)
    worst = Fraction(0)
    for _ in range(60):
        p = [Fraction(float(v)) for v in rng.uniform(-300, 300, 3)]
        a = int(rng.integers(0, 3))
        p[a] = Fraction(int(rng.choice([-257, -256, -255, -1, 0, 1, 5, 255, 256, 257])))
        lo, hi = list(p), list(p)
        lo[a], hi[a] = p[a] - step, p[a] + step
        worst = max(worst, abs(tr.noise(tables, lo) - tr.noise(tables, hi)), abs(tr.noise(tables, lo) - tr.noise(tables, p)))
    print(f"largest jump across a lattice plane: {float(worst):.3e}")
    assert worst <= Fraction(1, 10 ** 25)


def test_noise_vanishes_on_the_lattice_and_is_bounded(tables):
    """At a lattice point only corner (0, 0, 0) has weight and its weight vector is zero; and
    |noise| <= sqrt 3: a convex combination of dot products of a unit vector with a vector in the unit cube."""
    rng = np.random.default_rng(4)
    for p in rng.integers(-300, 300, (40, 3)):
        assert tr.noise(tables, p.astype(np.float64)) == 0
    big = max(abs(tr.noise(tables, p)) for p in rng.uniform(-300, 300, (300, 3)))
    print(f"largest |noise| on 300 points: {float(big):.4f}")
    assert 0.3 < big <= Fraction(tr.SQRT3)


# ---- the tables as perlin.rs:13-30, 110-129 make them ---------------------------------------------------------
def _flattened_tables(world):
    soa = world.flatten()
    n = soa.n_perlin
    ranvec = np.ctypeslib.as_array(ctypes.cast(soa.perlin_ranvec, ctypes.POINTER(ctypes.c_double)), (n, 256, 3)).copy()
    perm = np.ctypeslib.as_array(ctypes.cast(soa.perlin_perm, ctypes.POINTER(ctypes.c_int32)), (n, 3, 256)).copy()
    return ranvec, perm


@pytest.mark.parametrize("source", ["scene2", "scene7", "custom1", "custom2", "custom7", "custom99"])
def test_perlin_tables(rt, source):
    """ranvec: unit vectors (perlin.rs:17). perm: `permute` (perlin.rs:122-129) walks i from 255 down,
    draws target in [0, i], and writes p[i] = target (the index itself, not the value it held: Q10) and
    then p[target] = the old p[i]. Every later step i' < i writes only p[i'] and p[target'] with
    target' <= i' < i, so after step i nothing writes p[i] again. Where target != i the table therefore
    ends with p[i] = target < i. Where target == i the second write undoes the first and p[i] keeps what
    it held, which an earlier step may have moved down from a higher index: so p[i] <= i does NOT hold
    for every i (it never needs to at i = 0, where target is always 0), only for all i but those with
    target_i == i. Their number is a sum of independent draws with probabilities 1 / (i + 1): its mean is
    H_256 = 6.12, and by the Chernoff bound exp(mu (d - (1 + d) ln(1 + d))) with 1 + d = 24 / 6.12 it
    reaches 24 with probability under 4e-7 per table. A true shuffle has p[i] > i at about 127 places
    (and never repeats a value), so `at most 23 entries above their index` separates the two, and a
    table of draws target_i <= i almost surely repeats a value."""
    if source.startswith("scene"):
        world = rt.World(1).build_scene(int(source[5:]))
    else:
        world = rt.World(int(source[6:]))
        world.push(world.sphere(world.lambertian(world.noise(4.0)), (0.0, 0.0, 0.0), 1.0))
        world.push(world.sphere(world.lambertian(world.noise(0.1)), (3.0, 0.0, 0.0), 1.0))
    ranvec, perm = _flattened_tables(world)
    assert len(ranvec) == (1 if source.startswith("scene") else 2)
    ulp4 = Fraction(4, 2 ** 52)
    worst = Fraction(0)
    for v in ranvec.reshape(-1, 3):
        n2 = sum(Fraction(float(c)) ** 2 for c in v)
        assert (1 - ulp4) ** 2 <= n2 <= (1 + ulp4) ** 2, v
        worst = max(worst, abs(n2 - 1) / 2)
    print(f"{source}: largest | |ranvec| - 1 | = {float(worst) * 2 ** 52:.2f} ulp")
    assert ((perm >= 0) & (perm <= 255)).all()
    above = (perm > np.arange(256)).sum(axis=-1)
    print(f"{source}: entries above their index per table {above.reshape(-1).tolist()}, distinct values "
          f"{[len(np.unique(t)) for t in perm.reshape(-1, 256)]}")
    assert (above <= 23).all()
    assert any(len(np.unique(t)) < 256 for t in perm.reshape(-1, 256))
    if not source.startswith("scene"):
        assert not np.array_equal(ranvec[0], ranvec[1]) and not np.array_equal(perm[0], perm[1])


# ---- the oracle against the reference ----------------------------------------------------------------------
def test_oracle_matches_the_reference_on_plane_points(generated):
    arrays, _ = generated
    share = 0.0
    for tex in tp.PLANE_TEXTURES:
        for axis in range(3):
            s = tp.plane_set(tex, axis)
            world = tp.plane_world(ob.OracleWorld(tp.SCENE_SEED), tex, axis)
            rec = world.hit(s.rays, tp.QUERY_SEED, 0)
            world.close()
            assert (rec["hit"] != 0).all() and (rec["t"] == 1.0).all() and np.array_equal(rec["p"], s.pts), (tex, axis)
            # Lambertian (handle 1) on even entries of K, DiffuseLight (2) on odd ones
            assert np.array_equal(rec["mat"], 1 + np.array([tp.K.index(k) for k in s.pts[:, tp.PLANE_AXIS[axis]]]) % 2)
            scale_z = tp.NOISE_SCALES.get(tex, 0.0) * s.pts[:, 2]
            share = max(share, tp.judge(rec["albedo"], arrays, f"{tex}_{axis}", scale_z, s.classes, s.cls, f"{tex} axis {axis}"))
            if tex == "checker":
                code = arrays[f"{tex}_{axis}.code"][s.pinned]
                assert 0.2 < (code == tp.CODE_ODD).mean() < 0.8
    print(f"largest noise error: {share:.4f} of the bar")
    assert share <= 0.25, "over a quarter of the derived bar: revisit the derivation or the code"


def test_oracle_matches_the_reference_on_carriers(generated):
    arrays, _ = generated
    for name, (build, make_set) in tp.CARRIER_WORLDS.items():
        rays, derived = make_set()
        world = ob.OracleWorld(tp.SCENE_SEED)
        carriers = build(world)
        rec = world.hit(rays, tp.QUERY_SEED, 0)
        world.close()
        names = sorted({c.name for c in carriers.values()} | {"miss"})
        cls = np.array([names.index(carriers[int(m)].name if h else "miss") for m, h in zip(rec["mat"], rec["hit"])])
        share = tp.judge(rec["albedo"], arrays, name, tp.NOISE_CARRIER_SCALE * rec["p"][:, 2], names, cls, name)
        assert share <= 0.25
        if name == "spheres":          # the records derived by hand (texture_points.DERIVED_SPHERE_RAYS)
            code = arrays["spheres.code"][:len(tp.DERIVED_SPHERE_RAYS)]
            assert [(int(c) % tp.IMG_W, int(c) // tp.IMG_W) for c in code] == [t for _, t in tp.DERIVED_SPHERE_RAYS]
        elif name == "nested":         # the medium's image texel is (0, h - 1) wherever it is hit
            medium = (rec["hit"] != 0) & (rec["mat"] == 4)
            assert medium.sum() >= 20 and (arrays["nested.code"][medium] == (tp.IMG_H - 1) * tp.IMG_W).all()
            assert derived.sum() == 40 and (rec["mat"][derived] == 1).all() and (rec["t"][derived] == 1.0).all()


# ---- hard points of the shared transcendentals, mpmath as truth ----------------------------------------------
def test_sin_cos_next_to_multiples_of_half_pi():
    """rt__rem_pio2's hard inputs: the doubles within 3 ulp of k pi / 2, over the whole claimed domain
    |x| < 2^20 pi / 2 to its last k, and |x| = 65536 +- 8 ulp. The header's claims: 2 ulp, every sign right."""
    x = tp.hard_trig_points()
    assert len(x) > 130000 and np.abs(x).max() < tp.SIN_DOMAIN
    assert np.abs(x).max() > float((tp.K_LAST - 1) * tp.PI / 2)
    s_hi, s_lo = tr.truth(mpmath.sin, x)
    c_hi, c_lo = tr.truth(mpmath.cos, x)
    s, c, sg = ob.evaluate(0, x), ob.evaluate(1, x), ob.evaluate(12, x)
    es, ec = tr.ulp_error(s, s_hi, s_lo), tr.ulp_error(c, c_hi, c_lo)
    print(f"rt_sin {es.max():.3f} ulp, rt_cos {ec.max():.3f} ulp on {len(x)} doubles next to k pi / 2; smallest |sin| "
          f"{np.abs(s_hi).min():.3e}; rt_sin_sign answers 2 on {int((sg == 2).sum())}")
    assert es.max() <= 2.0 and ec.max() <= 2.0
    assert np.array_equal(np.sign(s), np.sign(s_hi)) and np.array_equal(np.sign(c), np.sign(c_hi))
    known = sg != 2
    assert np.array_equal(sg[known], np.sign(s_hi)[known]) and (np.abs(s_hi[~known]) < 2.0 ** -300).all()


def test_where_the_sine_domain_ends():
    """Inside |x| < 2^20 pi / 2 the test above finds no error over 2 ulp. Past it accuracy is not claimed
    (rt_abi.h says so to callers): this test asserts only that results there repeat and, up to the
    magnitudes stated at its end, are finite, and fixes that the limit is real: on the doubles within 3 ulp of m pi between the end of the domain
    and 3.2e7 the reduction does lose the sign of the sine somewhere, so the header's limit may not be
    dropped without a Payne-Hanek tail. The first failures this set finds are printed; DESIGN.md records them."""
    x = tp.beyond_trig_points()
    s, sg = ob.evaluate(0, x), ob.evaluate(12, x)
    assert np.isfinite(s).all() and (np.abs(s) <= 1.0).all()
    assert np.array_equal(s, ob.evaluate(0, x)) and np.array_equal(sg, ob.evaluate(12, x))
    hi, lo = tr.truth(mpmath.sin, x)
    wrong = np.sign(s) != np.sign(hi)
    off = tr.ulp_error(s, hi, lo) > 2.0
    sign_fn = (sg != 2) & (sg != np.sign(hi))
    for label, bad in (("rt_sin over 2 ulp", off), ("rt_sin's sign wrong", wrong), ("rt_sin_sign wrong", sign_fn)):
        print(f"{label}: {int(bad.sum())} of {len(x)}, first at |x| = {np.abs(x[bad]).min() if bad.any() else None!r}")
    assert wrong.any() and np.abs(x[wrong | off | sign_fn]).min() >= tp.SIN_DOMAIN
    # further out: a sine within [-1, 1] while |x| <= 2^40, a finite value while |x| <= 2^100 (the reduction's
    # remainder grows with |x| and the kernels' polynomials with its 13th power: 4e24 at 2^60), and from about
    # 2^120 infinities and NaN. Every one of them repeats.
    rng = np.random.default_rng(6)
    for top, bounded in ((40, True), (100, False)):
        far = 2.0 ** rng.uniform(25, top, 4000) * rng.choice([-1.0, 1.0], 4000)
        v = np.concatenate([ob.evaluate(0, far), ob.evaluate(1, far)])
        assert np.isfinite(v).all() and (not bounded or (np.abs(v) <= 1.0).all()), top
    far = np.array([2.0 ** 60, 1e300, -1.7e308])
    for fn in (0, 1, 12):
        assert np.array_equal(ob.evaluate(fn, far), ob.evaluate(fn, far), equal_nan=True)
    assert np.isin(ob.evaluate(12, far), [-1, 1, 2]).all()


def test_atan2_on_the_axes_and_at_signed_zeros():
    """IEEE 754 / C99 F.9.1.4: atan2(+-0, x > 0 or +0) = +-0; atan2(+-0, x < 0 or -0) = +-pi;
    atan2(y, +-0) = +-pi / 2 by y's sign. pi and pi / 2 are the correctly rounded doubles."""
    y, x = tp.hard_atan2_points()
    got = ob.evaluate(3, y, x)
    pi = float(mpmath.mp.pi)
    for a, b, g in zip(y, x, got):
        neg_x = np.signbit(b)
        if a == 0.0:
            want = np.copysign(pi if neg_x else 0.0, a)
        else:
            assert b == 0.0
            want = np.copysign(pi / 2, a)
        assert g == want and np.signbit(g) == np.signbit(want), (a, b, g, want)


def test_acos_and_log_at_their_edges():
    x = tp.hard_acos_points()
    hi, lo = tr.truth(mpmath.acos, x)
    got = ob.evaluate(4, x)
    e = np.where(hi == 0.0, np.where(got == 0.0, 0.0, np.inf), tr.ulp_error(got, hi, np.where(hi == 0.0, 0.0, lo)))
    print(f"rt_acos at +-1, 1 - 2^-53, +-0.5: {e.max():.3f} ulp")
    assert e.max() <= 2.0 and got[0] == 0.0
    assert ob.evaluate(4, np.array([-1.0]))[0] == float(mpmath.mp.pi)
    x = tp.hard_log_points()
    hi, lo = tr.truth(mpmath.log, x)
    e = tr.ulp_error(ob.evaluate(2, x), hi, lo)
    print(f"rt_log next to 1: {e.max():.3f} ulp on {len(x)} points")
    assert e.max() <= 2.0 and ob.evaluate(2, np.array([1.0]))[0] == 0.0
