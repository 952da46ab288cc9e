"""The primary-candidate table (csrc/primary_candidates.hpp, RT_OPT_PRIMARY_CANDIDATES) on the CPU:
every primitive a primary ray of a pixel hits first is in the pixel's list, or the pixel is
flagged "walk".

The table is the host twin's (rt_primary_candidates_host: the build_pixel the device kernel runs,
over the tables an upload gives the device). The first hit is a numpy restatement of the oracle's
primary rays: per (pixel, sample) the path stream's draws (oracle_binding.pstream) in the order the
camera takes them — two jitter draws, random_in_unit_disk's tries, the ray time — mapped as the
oracle maps them (orc_eval fn 10 and 11), then oracle.c's sphere_hit over every leaf primitive
with t in (0.001, closest so far), a moving sphere at its centre for the ray's time. (The time's
scale is (time1 - time0) / (1 - 2^-52) without rand's last-ulp adjustment: a first hit does not
turn on it.)

Worlds: the random scene and the spheres-only worlds of tests/generated_worlds.py (moving spheres
under shutters beside the camera's, a camera inside a glass sphere). Frames of 48x32x6, 37x21x17
and 9x5x1. Cameras: the world's own, lens radius 0, time0 == time1, and one inside the random
scene's sphere field.

The cap. At most 10 % of a frame's pixels may be flagged. A record holds 7 candidates (16 bytes:
a count and seven 16-bit leaf slots), and K is that 7: with it the random scene at the size it is
rendered at flags 1.5 % (1200x800; the gate below prints it). A pixel of a 48-pixel-wide frame
under the preset's 20 degree lens is 25 times as wide and covers a dozen of the small spheres,
so those frames are taken through longer lenses aimed at the rim of the large metal sphere and the
small spheres before it (VFOV below, found with the host builder before K was fixed: the widest of
6, 5, 4, 3, 2.5, 2 and 1.25 degrees that holds the cap under every camera of the frame) — the frame
changes, not the cap.
"""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import generated_worlds as gw
from tests import oracle_binding as ob

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust-ray-tracing-in-a-weekend_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
MAIN_SOURCES = [os.path.join(REPO, "tests", "primary_candidates_main.cpp")] + \
    [os.path.join(CSRC, f) for f in ("primary_candidates_host.cpp", "scene_model.cpp", "flatten.cpp", "bvh_build.cpp",
                                     "scene_lower.cpp")]

PRIM = np.dtype([("kind", "<i4"), ("mat", "<i4"), ("a", "<i4"), ("b", "<i4"), ("p", "<f8", (10,))])
SPHERE, MOVING = 0, 1
WALK = 0xFFFF
K = 7
CAP = 0.10
SIZES = [(48, 32, 6), (37, 21, 17), (9, 5, 1)]
T_MIN = 0.001


def leaf_prims(soa):
    import ctypes

    def table(ptr, n, dt):
        return np.frombuffer(ctypes.string_at(ptr, n * dt.itemsize), dtype=dt).copy() if n else np.zeros(0, dt)
    prims = table(soa.prims, soa.n_prims, PRIM)
    refs = table(soa.prim_refs, soa.n_prim_refs, np.dtype("<i4"))
    return prims[refs]      # by leaf slot


def primary_rays(cam, W, H, spp, seed=1):
    """(origin, direction, time) of every (pixel, sample), (H, W, spp, 3) and (H, W, spp)."""
    n_tries = 48
    n = 2 + 2 * n_tries + 1
    bits = np.empty((H, W, spp, n), dtype=np.uint64)
    for y in range(H):
        for x in range(W):
            for s in range(spp):
                bits[y, x, s] = ob.pstream(seed, y * W + x, s, n)
    as_f64 = bits.view(np.float64)
    unit = ob.evaluate(10, as_f64[..., :2].reshape(-1)).reshape(H, W, spp, 2)
    m11 = ob.evaluate(11, as_f64[..., 2:2 + 2 * n_tries].reshape(-1)).reshape(H, W, spp, n_tries, 2)
    inside = (m11 ** 2).sum(-1) < 1.0
    assert inside.any(-1).all(), "a lens draw rejected %d times" % n_tries
    first = inside.argmax(-1)
    disk = np.take_along_axis(m11, first[..., None, None], axis=3)[..., 0, :]
    tbits = np.take_along_axis(bits, (2 + 2 * (first + 1))[..., None], axis=3)[..., 0]
    v01 = ((tbits >> np.uint64(12)) | np.uint64(0x3FF0000000000000)).view(np.float64) - 1.0
    time = v01 * ((cam.time1 - cam.time0) / (1.0 - 2.0 ** -52)) + cam.time0
    ys, xs = np.mgrid[0:H, 0:W]
    u = (xs[..., None] + unit[..., 0]) / (W - 1)
    v = (ys[..., None] + unit[..., 1]) / (H - 1)
    vec = lambda f: np.array(list(getattr(cam, f)))
    rd = disk * cam.lens_radius
    off = rd[..., 0:1] * vec("u") + rd[..., 1:2] * vec("v")
    origin = vec("origin") + off
    direction = vec("lower_left_corner") + u[..., None] * vec("horizontal") + v[..., None] * vec("vertical") - vec("origin") - off
    return origin, direction, time


def first_hit_slots(leaf, origin, direction, time):
    """The leaf slot of each ray's closest hit, -1 for none (oracle.c sphere_hit, moving_center)."""
    assert (leaf["kind"] <= MOVING).all()
    p = leaf["p"]
    moving = leaf["kind"] == MOVING
    t0 = np.where(moving, p[:, 8], 0.0)
    t1 = np.where(moving, p[:, 9], 1.0)
    vel = np.where(moving[:, None], p[:, 5:8], 0.0)
    o = origin.reshape(-1, 3)
    d = direction.reshape(-1, 3)
    tm = time.reshape(-1)
    best = np.full(o.shape[0], -1)
    best_t = np.full(o.shape[0], np.inf)
    with np.errstate(all="ignore"):
        for j in range(len(leaf)):
            c = p[j, 0:3] + vel[j] * ((tm[:, None] - t0[j]) / (t1[j] - t0[j]))
            oc = o - c
            a = (d * d).sum(-1)
            half_b = (oc * d).sum(-1)
            cc = (oc * oc).sum(-1) - p[j, 3] * p[j, 3]
            disc = half_b * half_b - a * cc
            sq = np.sqrt(np.where(disc >= 0, disc, 0.0))
            r0, r1 = (-half_b - sq) / a, (-half_b + sq) / a
            ok0 = ~((r0 < T_MIN) | (best_t < r0))
            ok1 = ~((r1 < T_MIN) | (best_t < r1))
            hit = (disc >= 0) & (ok0 | ok1)
            t = np.where(ok0, r0, r1)
            best = np.where(hit, j, best)
            best_t = np.where(hit, t, best_t)
    return best.reshape(time.shape)


def check_containment(rt, soa, cam, W, H, spp, label):
    rec, info = rt.primary_candidates_host(soa, cam, W, H, K)
    assert info.slots == K and info.pixels == W * H
    share = info.flagged / info.pixels
    listed = info.pixels - info.flagged
    print(f"{label} {W}x{H}x{spp}: flagged {info.flagged} of {info.pixels} ({share:.3f}), candidates mean "
          f"{info.candidates / max(listed, 1):.2f} max {info.max_candidates}")
    assert share <= CAP, f"{label}: {share:.3f} of the frame's pixels are flagged"
    leaf = leaf_prims(soa)
    hit = first_hit_slots(leaf, *primary_rays(cam, W, H, spp))
    n = rec[..., 0].astype(np.int64)
    flagged = n == WALK
    slots = np.where(np.arange(1, 8) <= np.where(flagged, 0, n)[..., None], rec[..., 1:].astype(np.int64), -2)
    inside = (slots[:, :, None, :] == hit[..., None]).any(-1)
    bad = (hit >= 0) & ~flagged[..., None] & ~inside
    assert hit.max() >= 0, f"{label}: no primary ray hits anything"
    assert not bad.any(), (f"{label}: {int(bad.sum())} first hits outside their pixel's list; the first at (y, x, s) = "
                           f"{tuple(int(i) for i in np.argwhere(bad)[0])}: slot {int(hit[tuple(np.argwhere(bad)[0])])}")
    return share


# ---- the random scene -----------------------------------------------------------------------------
# vfov per frame width (module docstring); from the preset's (13, 2, 3)
VFOV = {48: 4.0, 37: 3.0, 9: 1.25}
LOOK_AT = (4.0, 0.7, 0.8)


def random_scene_camera(rt, kind, W, H):
    look_from, look_at, aperture, t0, t1 = (13.0, 2.0, 3.0), LOOK_AT, 0.1, 0.0, 1.0
    vfov = VFOV[W]
    if kind == "pinhole":
        aperture = 0.0
    elif kind == "one_time":
        t0 = t1 = 0.5
    elif kind == "inside_field":       # between the small spheres, looking along the ground at the big ones
        look_from, look_at = (6.5, 0.45, 2.4), (4.0, 1.0, 0.0)
        aperture, vfov = 0.02, 10.0
    return rt.camera_new(look_from, look_at, (0.0, 1.0, 0.0), vfov, W / H, aperture, 10.0, t0, t1)


@pytest.fixture(scope="module")
def random_soa(rt):
    world = rt.World(1).build_scene(0)
    return world, world.flatten(rt.RT_ACCEL_SAH)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("kind", ["preset", "pinhole", "one_time", "inside_field"])
def test_random_scene_first_hits_are_listed(rt, random_soa, kind, size):
    W, H, spp = size
    check_containment(rt, random_soa[1], random_scene_camera(rt, kind, W, H), W, H, spp, f"random scene, {kind}")


# ---- the spheres-only generated worlds ------------------------------------------------------------
SPHERES_ONLY = [c for c in gw.SUPPORTED if c.name in ("camera_time_outside", "camera_time_inside", "inside_glass")]
GEN_VFOV = {48: 20.0, 37: 20.0, 9: 10.0}


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("case", SPHERES_ONLY, ids=[c.name for c in SPHERES_ONLY])
def test_generated_world_first_hits_are_listed(rt, case, size):
    W, H, spp = size
    b = gw.build(rt, case)
    soa = b.tw.product.flatten(rt.RT_ACCEL_SAH)
    cam = rt.camera_new(case.look_from, case.look_at, (0.0, 1.0, 0.0), GEN_VFOV[W], W / H, case.aperture, case.focus,
                        case.time[0], case.time[1])
    check_containment(rt, soa, cam, W, H, spp, case.name)


def test_spheres_only_worlds_are_what_the_name_says(rt):
    assert len(SPHERES_ONLY) == 3
    for case in SPHERES_ONLY:
        b = gw.build(rt, case)      # (the tables are the world's: it stays alive while they are read)
        leaf = leaf_prims(b.tw.product.flatten(rt.RT_ACCEL_SAH))
        assert len(leaf) >= 24 and (leaf["kind"] <= MOVING).all()


# ---- flags ------------------------------------------------------------------------------------------
def test_a_pixel_is_flagged_for_an_unknown_kind_a_short_record_or_an_uncovered_camera(rt, random_soa):
    W, H = 48, 32
    cam = random_scene_camera(rt, "preset", W, H)
    full, info = rt.primary_candidates_host(random_soa[1], cam, W, H, K)
    one, info1 = rt.primary_candidates_host(random_soa[1], cam, W, H, 1)
    n, n1 = full[..., 0].astype(int), one[..., 0].astype(int)
    assert ((n1 == WALK) == ((n == WALK) | (n > 1))).all()      # k = 1 flags exactly the pixels with more than one
    assert info1.flagged > info.flagged and info1.max_candidates <= 1
    assert (one[n1 == 1][:, 1] == full[n1 == 1][:, 1]).all()
    # a camera focused on its own lens: no bound, every pixel walks
    near = rt.camera_new((13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 20.0, W / H, 2.0, 0.5, 0.0, 1.0)
    rec, inf = rt.primary_candidates_host(random_soa[1], near, W, H, K)
    assert inf.flagged == W * H and (rec[..., 0] == WALK).all()
    # a one-pixel-wide frame has no jitter divisor
    rec, inf = rt.primary_candidates_host(random_soa[1], cam, 1, 5, K)
    assert inf.flagged == 5
    # a world with a rect: the pixels whose cone reaches its leaf are flagged, the others listed
    case = next(c for c in gw.SUPPORTED if c.name == "materials")
    b = gw.build(rt, case)
    rec, inf = rt.primary_candidates_host(b.tw.product.flatten(rt.RT_ACCEL_SAH), gw.camera(rt, case, W, H), W, H, K)
    assert 0 < inf.flagged


# ---- the stand-alone host program: the gate's figures, and the sanitizers ----------------------------
def _build_main(exe, flags):
    b = subprocess.run([CLANG, "-std=c++17", "-ffp-contract=off", *flags, "-I" + os.path.join(REPO, "include"), "-I" + CSRC,
                        *MAIN_SOURCES, "-o", exe], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]


def test_gate_figures_at_the_headline_geometry(tmp_path):
    """The estimate behind the option holds only while the lists are short and few pixels walk: the
    candidate count's mean at most 4, the flagged share a few percent, at 1200x800."""
    exe = str(tmp_path / "primary_candidates_main")
    _build_main(exe, ["-O2"])
    r = subprocess.run([exe, "1200", "800", str(K), "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    d = json.loads(r.stdout)
    print(f"1200x800: candidates mean {d['mean_candidates']:.2f} max {d['max_candidates']}, flagged share {d['flagged_share']:.4f}, "
          f"table {d['table_bytes'] / 2**20:.1f} MiB")
    assert d["mean_candidates"] <= 4.0 and d["flagged_share"] <= 0.05 and d["table_bytes"] == 1200 * 800 * 16


def test_host_program_is_clean_under_asan_and_ubsan(tmp_path):
    """The program itself is instrumented and run directly (nothing is preloaded): the 37x21 frame,
    17 rays per pixel against a brute-force closest hit, and K forced to 1."""
    exe = str(tmp_path / "primary_candidates_main_san")
    _build_main(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for k in (K, 1):
        r = subprocess.run([exe, "37", "21", str(k), "17"], capture_output=True, text=True, env=env, timeout=300)
        report = r.stdout + r.stderr
        assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
        assert r.returncode == 0, report[-4000:]
        d = json.loads(r.stdout)
        assert d["contained"] and d["hits"] > 0 and d["max_candidates"] <= k
