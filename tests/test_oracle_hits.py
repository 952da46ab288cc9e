"""The oracle's caller-ray entries (orc_world_hit, orc_scene_hit: oracle/oracle.h) and the caller-ray
sets chosen with them (tests/oracle_rays.py), on the CPU. tests/test_gpu_trace_rays_oracle.py holds
rt_trace_rays to these; here they are held to what already stands:

- the numpy closest hit of tests/query_reference.py on the two SIMPLE worlds and its 1,000 rays each:
  hit / miss, winner and front flag equal, t, p and n within 1e-12 (1 + |x|) — two f64 restatements of
  the same formulas with contraction off; 1e-12 is four orders over roundoff and three under the GPU bar;
- the oracle's own render path: over the LightTwin worlds the albedo of rt_camera_rays' rays, the
  background put in on a miss, is OracleWorld.render at max_depth 1;
- records asserted from hittable.rs by hand: set_face_normal applied again at every level of a
  translate / rotate_y chain (:232-244, :386-415), a medium's (1, 0, 0) rotated and flipped by them,
  a medium's rec1.t clamped to t_min and then to 0 (:417-473);
- the sets: deterministic, full, every interval class present, hits and misses, phase-function hits;
- tests/oracle_hit_main.c with oracle.c under ASan and UBSan, run directly, against the same program
  linked to liboracle.so.
"""
import os
import subprocess

import numpy as np
import pytest

from tests import features_reference as fr
from tests import oracle_binding as ob
from tests import oracle_rays
from tests import query_reference as qr
from tests import test_gpu_features as tf
from tests import test_gpu_trace_rays_oracle as worlds
from tests.test_gpu_parity import assert_parity

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
SAN_FLAGS = ["-std=c99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
             "-fno-fast-math", "-fno-math-errno"]


def _simple_oracle(prims, materials):
    """features_reference.build_simple's world in the oracle: primitive i carries material i + 1."""
    w = ob.OracleWorld(1)
    for prim, kind in zip(prims, materials):
        c = prim[-1]
        m = {"lambertian": lambda: w.lambertian(w.solid(*c)), "metal": lambda: w.metal(c, 0.3),
             "dielectric": lambda: w.dielectric(1.5), "light": lambda: w.diffuse_light(w.solid(*c))}[kind]()
        if prim[0] == "sphere":
            w.push(w.sphere(m, prim[1], prim[2]))
        else:
            _, axis, a0, a1, b0, b1, k, _ = prim
            w.push((w.xy_rect, w.xz_rect, w.yz_rect)[axis](m, a0, a1, b0, b1, k))
    return w


@pytest.mark.parametrize("name", list(tf.SIMPLE))
def test_world_hit_is_the_numpy_closest_hit(name):
    prims, mats, _ = tf.SIMPLE[name]
    o, d, t_min, t_max, cls = qr.caller_rays(prims)
    ref = qr.closest_hit(prims, o, d, t_min, t_max)
    got = _simple_oracle(prims, mats).hit(qr.as_rays(ob.ORC_RAY, o, d, t_min, t_max), seed=1, bounce=0)
    hit = np.isfinite(ref["t"])
    assert np.array_equal(got["hit"] != 0, hit) and 200 < hit.sum() < 900
    assert np.isposinf(got["t"][~hit]).all()
    for f in ("p", "n", "albedo", "front_face", "mat", "top"):
        assert (got[f][~hit] == 0).all(), f
    assert np.array_equal(got["top"][hit], ref["index"][hit]) and np.array_equal(got["mat"][hit], ref["index"][hit] + 1)
    assert np.array_equal(got["front_face"] != 0, ref["front"])
    for f in ("t", "p", "n"):
        a, b = got[f][hit], ref[f][hit]
        err = float(np.max(np.abs(a - b) / (1.0 + np.abs(b))))
        print(f"{name} {f}: max |oracle - numpy| / (1 + |numpy|) = {err:.3e}")
        assert err <= 1e-12, f
    colour = np.array([(1.0, 1.0, 1.0) if m == "dielectric" else p[-1] for p, m in zip(prims, mats)])
    assert np.array_equal(got["albedo"][hit], colour[ref["index"][hit]])


@pytest.mark.parametrize("name", list(tf.WORLDS))
def test_albedo_is_the_oracles_render_at_depth_one(rt, monkeypatch, name):
    W, H = 37, 21
    tw, view = tf._world(rt, monkeypatch, name)
    cam = tf._camera(rt, view, W, H)
    got = tw.oracle.hit(rt.camera_rays(cam, W, H, 1, 0), seed=1, bounce=0)
    miss = got["hit"] == 0
    assert 0 < int(miss.sum()) < W * H
    albedo = np.where(miss[:, None], np.array(tf.BG), got["albedo"]).reshape(H, W, 3)
    ref = tw.oracle.render(fr.cam24(cam), tf.BG, W, H, 1, max_depth=1)
    assert_parity(albedo, ref, f"orc_world_hit albedo, {name}")


def test_scene_hit_is_world_hit_over_the_built_in_scene(rt):
    """orc_scene_hit builds what orc_render builds: scene 5's primary rays get the albedo its
    LightTwin-free render cannot show, so the check is structural — every hittable of the scene wins
    some ray, with the materials cornell_box_scene registers (red 1, white 2, green 3, light 4)."""
    W, H = 48, 32
    cam = rt.scene_camera(5, W, H)[0]
    got = ob.scene_hit(5, rt.camera_rays(cam, W, H, 1, 0), seed=1)
    assert (got["hit"] != 0).sum() > W * H // 2
    got = got[got["hit"] != 0]
    assert sorted(set(got["top"].tolist())) == [0, 1, 2, 3, 4, 5, 6, 7]
    want = {0: 3, 1: 1, 2: 4, 3: 2, 4: 2, 5: 2, 6: 2, 7: 2}
    assert all(want[t] == m for t, m in zip(got["top"].tolist(), got["mat"].tolist()))
    with pytest.raises(RuntimeError):
        ob.scene_hit(8, np.zeros(1, dtype=ob.ORC_RAY))


# ---- records asserted from hittable.rs by hand ---------------------------------------------------------
def _one(o, d, t_min=0.001, t_max=np.inf):
    r = np.zeros(1, dtype=ob.ORC_RAY)
    r["o"], r["d"], r["t_min"], r["t_max"] = o, d, t_min, t_max
    return r


def test_an_instanced_box_is_front_facing_from_inside():
    """From inside a box the side's own set_face_normal (hittable.rs:308-384) turns the normal against
    the ray and clears front_face; RotateY and Translate then call set_face_normal again with that
    normal as the outward one (:386-415, :232-244), and a normal already against the ray is front-facing.
    The ray goes up to the top side, whose normal the rotation about y leaves alone."""
    s, c = np.sin(np.radians(30.0)), np.cos(np.radians(30.0))
    local = np.array([0.5, 1.0, 0.5])
    d = np.array([0.1, 1.0, 0.2]) * 0.7

    w = ob.OracleWorld(1)
    white = w.lambertian(w.solid(0.7, 0.7, 0.7))
    w.push(w.box((0.0, 0.0, 0.0), (1.0, 2.0, 1.0), white))
    top = w.hit(_one(local, d))[0]
    assert top["hit"] == 1 and top["front_face"] == 0 and top["n"].tolist() == [0.0, -1.0, 0.0]
    assert abs(top["t"] - 1.0 / d[1]) <= 1e-15 and abs(top["p"][1] - 2.0) <= 1e-15

    w = ob.OracleWorld(1)
    white = w.lambertian(w.solid(0.7, 0.7, 0.7))
    w.push(w.translate(w.rotate_y(w.box((0.0, 0.0, 0.0), (1.0, 2.0, 1.0), white), 30.0), (5.0, 0.0, -3.0)))
    o = np.array([c * local[0] + s * local[2], local[1], -s * local[0] + c * local[2]]) + np.array([5.0, 0.0, -3.0])
    inst = w.hit(_one(o, d))[0]
    assert inst["hit"] == 1 and inst["front_face"] == 1 and inst["n"].tolist() == [0.0, -1.0, 0.0]
    assert float(np.dot(inst["n"], d)) < 0.0
    assert abs(inst["t"] - 1.0 / d[1]) <= 1e-14 and abs(inst["p"][1] - 2.0) <= 1e-14
    assert np.abs(inst["p"] - (o + inst["t"] * d)).max() <= 1e-14


def _fog_world(wrap):
    """A unit sphere of medium at the origin, so dense (1e8) that every chord accepts within 3.7e-7 of its
    start; wrap(world, medium id) gives the hittable to push."""
    w = ob.OracleWorld(1)
    phase = w.isotropic(w.solid(0.5, 0.5, 0.5))
    w.push(wrap(w, w.constant_medium(w.sphere(phase, (0.0, 0.0, 0.0), 1.0), 1e8, phase)))
    return w


def test_a_medium_under_an_instance_gets_its_normal_rotated_and_flipped():
    """ConstantMedium::hit returns normal (1, 0, 0) and front_face true (hittable.rs:417-473). RotateY
    rotates it to (cos a, 0, -sin a) and turns it against its own (rotated) ray; Translate's
    set_face_normal turns it against the ray, so under translate(rotate_y(., 40)) the record has
    n = +-(cos 40, 0, -sin 40), the sign from d. For the three rays here the two levels agree, so the
    record is front-facing. Top-level the record keeps (1, 0, 0) whatever d is."""
    s, c = np.sin(np.radians(40.0)), np.cos(np.radians(40.0))
    axis = np.array([c, 0.0, -s])
    w = _fog_world(lambda w, fog: w.translate(w.rotate_y(fog, 40.0), (3.0, 0.0, 0.0)))
    signs = []
    for o, d in (((6.0, 0.0, 0.0), (-1.0, 0.0, 0.0)), ((3.0, 0.0, 4.0), (0.0, 0.0, -2.0)), ((3.0, 3.0, 0.1), (0.1, -1.0, 0.0)),
                 ((0.0, 0.0, 0.0), (1.5, 0.0, 0.0))):
        h = w.hit(_one(o, d))[0]
        sign = -np.sign(np.dot(axis, d))
        signs.append(sign)
        assert h["hit"] == 1 and h["front_face"] == 1
        assert np.abs(h["n"] - sign * axis).max() <= 1e-15 and float(np.dot(h["n"], d)) < 0.0, (d, h["n"])
    assert sorted(set(signs)) == [-1.0, 1.0]
    # Translate alone: (1, 0, 0) turned against the ray, and front_face says whether it had to be
    w = _fog_world(lambda w, fog: w.translate(fog, (0.0, 2.0, 0.0)))
    h = w.hit(_one((5.0, 2.0, 0.0), (-1.0, 0.0, 0.0)))[0]
    assert h["hit"] == 1 and h["front_face"] == 1 and h["n"].tolist() == [1.0, 0.0, 0.0]
    h = w.hit(_one((-5.0, 2.0, 0.0), (1.0, 0.0, 0.0)))[0]
    assert h["hit"] == 1 and h["front_face"] == 0 and h["n"].tolist() == [-1.0, 0.0, 0.0]
    # top-level: as ConstantMedium::hit wrote it
    w = _fog_world(lambda w, fog: fog)
    for o, d in (((5.0, 0.0, 0.0), (-1.0, 0.0, 0.0)), ((-5.0, 0.0, 0.0), (1.0, 0.0, 0.0))):
        h = w.hit(_one(o, d))[0]
        assert h["hit"] == 1 and h["front_face"] == 1 and h["n"].tolist() == [1.0, 0.0, 0.0]


def test_a_medium_entered_before_t_min_starts_at_zero():
    """Origin inside the boundary, whose entry is at about -0.5: rec1.t is raised to t_min when below it,
    compared with rec2.t, and then raised to 0 (hittable.rs:435-445). So with t_min = -5 or -0.25 the
    distance drawn is laid off from t = 0 — not from the entry and not from t_min — and with an interval
    wholly behind the origin the length inside comes out negative and nothing is hit, though the boundary
    is there."""
    w = _fog_world(lambda w, fog: fog)
    o, d = np.array([0.1, -0.2, 0.05]), np.array([0.6, 0.3, -1.9])
    for t_min in (-5.0, -0.25, 0.001):
        h = w.hit(_one(o, d, t_min=t_min))[0]
        start = max(t_min, 0.0)
        assert h["hit"] == 1 and start <= h["t"] <= start + 37e-8 / np.linalg.norm(d), (t_min, h["t"])
        assert np.abs(h["p"] - (o + h["t"] * d)).max() <= 1e-15
    assert w.hit(_one(o, d, t_min=-5.0, t_max=-0.001))[0]["hit"] == 0
    assert w.hit(_one(o, d, t_min=-0.25, t_max=-0.001))[0]["hit"] == 0
    assert w.hit(_one(o + 4.0 * d, d, t_min=-10.0, t_max=-0.001))[0]["hit"] == 0     # the whole boundary behind the origin


# ---- the sets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(worlds.WORLDS))
def test_caller_ray_sets(rt, name):
    w = worlds.world(rt, name)
    s = worlds.ray_set(rt, name)
    bounces = (0, 3) if name in worlds.MEDIA else (0,)
    again = oracle_rays.build_set(w.hit_fn, w.cam, worlds.POOL_W, worlds.POOL_H, worlds.TIME_RANGE, 20261021, bounces=bounces, rt=rt)
    assert again.rays.tobytes() == s.rays.tobytes() and again.cls.tobytes() == s.cls.tobytes()
    for b in bounces:
        assert again.ref[b].tobytes() == s.ref[b].tobytes()
    ref = s.ref[0]
    hit = ref["hit"] != 0
    fog = hit & worlds.is_phase(w, ref["mat"])
    counts = np.bincount(s.cls, minlength=7)
    print(f"{name}: redrew {100.0 * s.redrawn:.1f} % in {s.rounds} round(s); hits {int(hit.sum())}; classes {counts.tolist()}; "
          f"origin kinds {np.bincount(s.kind, minlength=3).tolist()}; medium hits {int(fog.sum())}; back faces {int((hit & (ref['front_face'] == 0)).sum())}")
    assert s.rays.shape == (oracle_rays.N_RAYS,) and len(ref) == oracle_rays.N_RAYS
    assert (counts >= 50).all() and len(counts) == 7
    assert 0.20 * oracle_rays.N_RAYS < hit.sum() < 0.95 * oracle_rays.N_RAYS
    if name in worlds.MEDIA:
        assert fog.sum() >= 30
    # the set is what it says: its answers are the oracle's for its rays, the ends of the time range are there,
    # directions are not normalised, keys are spread
    assert w.hit_fn(s.rays, 0).tobytes() == ref.tobytes()
    lo, hi = worlds.TIME_RANGE
    assert (s.rays["time"] == lo).sum() >= 20 and (s.rays["time"] == hi).sum() >= 20
    assert ((s.rays["time"] >= lo) & (s.rays["time"] <= hi)).all() and (s.rays["t_min"] <= s.rays["t_max"]).all()
    length = np.linalg.norm(s.rays["d"], axis=-1)
    assert length.min() >= 0.4 - 1e-12 and length.max() <= 2.5 + 1e-12 and np.ptp(length) > 1.5
    assert s.rays["key_pixel"].max() < 1 << 20 and s.rays["key_sample"].max() < 64 and len(set(s.rays["key_pixel"].tolist())) > 900
    short, past, after, window = (s.cls == k for k in (1, 2, 3, 4))
    first = w.hit_fn(_with_interval(s.rays, oracle_rays.T_MIN, np.inf), 0)
    assert (first["hit"][short | past | after | window] != 0).all()
    assert np.array_equal(ref["t"][past], first["t"][past])                         # just past the first hit: still it
    assert (ref["t"][after] > first["t"][after]).all() and (ref["t"][window] > first["t"][window]).all()
    # (a medium's t depends on t_min, so a window around a medium's second hit may hold another t or nothing)
    assert hit[window].sum() >= 0.5 * window.sum()
    assert (ref["t"][hit & (s.cls == 5)] < 0).any()                                 # hits behind the origin


def _with_interval(rays, t_min, t_max):
    r = rays.copy()
    r["t_min"], r["t_max"] = t_min, t_max
    return r


# ---- sanitizers -----------------------------------------------------------------------------------------
def test_hit_program_is_clean_under_asan_and_ubsan_and_prints_the_librarys_checksums(tmp_path):
    """tests/oracle_hit_main.c compiled together with oracle.c, instrumented, and run directly (nothing is
    preloaded), against the same program linked to the shared library the other tests load."""
    main_c, oracle_c = os.path.join(REPO, "tests", "oracle_hit_main.c"), os.path.join(REPO, "oracle", "oracle.c")
    san = str(tmp_path / "oracle_hit_main_san")
    b = subprocess.run([CLANG, *SAN_FLAGS, main_c, oracle_c, "-o", san, "-lm", "-lpthread"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([san], capture_output=True, text=True, env=env, timeout=300)
    report = r.stdout + r.stderr
    assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
    assert r.returncode == 0, report[-4000:]
    ob.lib()    # builds liboracle.so if it is missing or older than oracle.c
    plain = str(tmp_path / "oracle_hit_main")
    b = subprocess.run(["gcc", "-std=c99", "-O1", "-ffp-contract=off", main_c, ob.ORACLE_LIB, "-Wl,-rpath," + os.path.dirname(ob.ORACLE_LIB),
                        "-o", plain, "-lm"], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    want = subprocess.run([plain], capture_output=True, text=True, timeout=300)
    assert want.returncode == 0, want.stdout + want.stderr
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.stdout == want.stdout and len(lines) == 6
    assert all(" hits 0 " in l for l in lines if "misses only" in l) and sum(" hits 0 " in l for l in lines) == 2
