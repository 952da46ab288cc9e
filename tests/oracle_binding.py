"""ctypes binding of the CPU oracle (oracle/liboracle.so) — TEST INFRASTRUCTURE ONLY.

Used by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg as the
checker / CPU baseline; never by the product path.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from functools import lru_cache

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(REPO, "oracle")
# RT_ORACLE_LIB: another build of the same source (the sanitizer run, tests/test_sanitizers.py)
ORACLE_LIB = os.environ.get("RT_ORACLE_LIB", os.path.join(ORACLE_DIR, "build", "liboracle.so"))
EARTH_JPG = os.path.join(REPO, "assets", "earthmap.jpg")

SPLIT_ROWS, SPLIT_SAMPLES = 0, 1


class Params(ctypes.Structure):
    _fields_ = [("scene_id", ctypes.c_int), ("scene_seed", ctypes.c_uint64), ("render_seed", ctypes.c_uint64),
                ("width", ctypes.c_int), ("height", ctypes.c_int), ("spp", ctypes.c_int),
                ("max_depth", ctypes.c_int), ("spp_chunk", ctypes.c_int), ("row_begin", ctypes.c_int),
                ("row_stride", ctypes.c_int), ("threads", ctypes.c_int), ("split", ctypes.c_int),
                ("image_rgb", ctypes.c_void_p), ("image_w", ctypes.c_int), ("image_h", ctypes.c_int)]


class Stats(ctypes.Structure):
    _fields_ = [("casts", ctypes.c_uint64), ("samples", ctypes.c_uint64), ("seconds", ctypes.c_double)]


@lru_cache(maxsize=1)
def lib() -> ctypes.CDLL:
    src = os.path.join(ORACLE_DIR, "oracle.c")
    if not os.path.exists(ORACLE_LIB) or (os.path.exists(src) and
                                          os.path.getmtime(src) > os.path.getmtime(ORACLE_LIB)):
        subprocess.run(["make", "-C", ORACLE_DIR, "-s"], check=True)
    l = ctypes.CDLL(ORACLE_LIB)
    l.orc_render.argtypes = [ctypes.POINTER(Params), ctypes.c_void_p, ctypes.POINTER(Stats)]
    l.orc_render.restype = ctypes.c_int
    l.orc_scene_info.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                 ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)]
    l.orc_scene_info.restype = ctypes.c_int
    l.orc_eval.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                           ctypes.c_int]
    l.orc_eval.restype = ctypes.c_int
    l.orc_philox.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    l.orc_philox.restype = None
    l.orc_pstream.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    l.orc_pstream.restype = None
    l.orc_camera.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    l.orc_camera.restype = ctypes.c_int
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    for name, args in {"orc_world_create": [ctypes.c_uint64, P], "orc_world_texture": [P, I, P, P, D],
                       "orc_world_texture_image": [P, P, I, I],
                       "orc_world_material": [P, I, I, P, D, D], "orc_world_sphere": [P, I, P, D],
                       "orc_world_moving_sphere": [P, I, P, P, D, D, D], "orc_world_rect": [P, I, I, D, D, D, D, D],
                       "orc_world_box": [P, P, P, I], "orc_world_translate": [P, I, P], "orc_world_rotate_y": [P, I, D],
                       "orc_world_constant_medium": [P, I, D, I], "orc_world_bvh": [P, P, I, D, D],
                       "orc_world_push": [P, I], "orc_world_render": [P, ctypes.POINTER(Params), P, P, P, P]}.items():
        getattr(l, name).argtypes = args
        getattr(l, name).restype = I
    l.orc_world_destroy.argtypes = [P]
    l.orc_world_destroy.restype = None
    l.orc_world_hit.argtypes = [P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64, P, P]
    l.orc_world_hit.restype = I
    l.orc_scene_hit.argtypes = [I, ctypes.c_uint64, P, I, I, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64, P, P]
    l.orc_scene_hit.restype = I
    l.orc_write_color.argtypes = [P, I, ctypes.c_int64, P]
    l.orc_write_color.restype = I
    l.orc_write_ppm.argtypes = [P, I, I, I, ctypes.c_char_p]
    l.orc_write_ppm.restype = I
    return l


@lru_cache(maxsize=1)
def earth_texture() -> np.ndarray:
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(EARTH_JPG).convert("RGB"), dtype=np.uint8))


def render(scene_id: int, width: int, height: int, spp: int, max_depth: int = 50, scene_seed: int = 1,
           render_seed: int = 1, row_begin: int = 0, row_stride: int = 1, threads: int = 0,
           split: int = SPLIT_ROWS, spp_chunk: int = 0, return_stats: bool = False):
    """Mean radiance of the selected rows, shape (rows, width, 3) f64 (row k = row_begin + k*row_stride)."""
    img = earth_texture() if scene_id in (3, 7) else np.zeros((1, 1, 3), np.uint8)
    if threads <= 0:
        threads = min(8, os.cpu_count() or 1)
    n_rows = 0 if row_begin >= height else (height - row_begin + row_stride - 1) // row_stride
    if spp_chunk <= 0:
        spp_chunk = min(16, max(1, (spp + 15) // 16))   # the product's automatic chunking (launch_plan.cpp auto_chunk)
    p = Params(scene_id, scene_seed, render_seed, width, height, spp, max_depth, spp_chunk, row_begin, row_stride,
               threads, split, img.ctypes.data, img.shape[1], img.shape[0])
    out = np.zeros((n_rows, width, 3), dtype=np.float64)
    st = Stats()
    rc = lib().orc_render(ctypes.byref(p), out.ctypes.data, ctypes.byref(st))
    if rc != 0:
        raise RuntimeError(f"orc_render failed: {rc}")
    return (out, st) if return_stats else out


def write_color(rgb, samples_per_pixel: int = 1) -> np.ndarray:
    """The oracle's write_color (math.rs:119-132) channel values of f64 sums / means."""
    a = np.ascontiguousarray(rgb, dtype=np.float64)
    out = np.empty(a.shape, dtype=np.int32)
    if lib().orc_write_color(a.ctypes.data, samples_per_pixel, a.size // 3, out.ctypes.data) != 0:
        raise ValueError("orc_write_color")
    return out


def write_ppm(rgb, path: str, samples_per_pixel: int = 1) -> None:
    """The oracle's P3 writer (main.rs:472, 591-596): rgb height x width x 3, row 0 = bottom."""
    a = np.ascontiguousarray(rgb, dtype=np.float64)
    if lib().orc_write_ppm(a.ctypes.data, samples_per_pixel, a.shape[1], a.shape[0], str(path).encode()) != 0:
        raise RuntimeError("orc_write_ppm")


def scene_info(scene_id: int, scene_seed: int = 1):
    img = earth_texture()
    n_h, n_m, n_l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cs = ctypes.c_double()
    rc = lib().orc_scene_info(scene_id, scene_seed, img.ctypes.data, img.shape[1], img.shape[0],
                              ctypes.byref(n_h), ctypes.byref(n_m), ctypes.byref(n_l), ctypes.byref(cs))
    if rc != 0:
        raise RuntimeError("orc_scene_info failed")
    return {"n_hittables": n_h.value, "n_materials": n_m.value, "n_leaf_prims": n_l.value, "checksum": cs.value}


def evaluate(fn: int, x, y=None, z=None) -> np.ndarray:
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(x if y is None else y, dtype=np.float64)
    z = np.ascontiguousarray(x if z is None else z, dtype=np.float64)
    out = np.empty_like(x)
    if lib().orc_eval(fn, x.ctypes.data, y.ctypes.data, z.ctypes.data, out.ctypes.data, x.size) != 0:
        raise ValueError(fn)
    return out


def philox(ctr, key) -> np.ndarray:
    c = np.ascontiguousarray(ctr, dtype=np.uint32)
    k = np.ascontiguousarray(key, dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    lib().orc_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return out


def camera(scene_id: int, width: int, height: int) -> np.ndarray:
    out = np.zeros(24, dtype=np.float64)
    if lib().orc_camera(scene_id, width, height, out.ctypes.data) != 0:
        raise ValueError(scene_id)
    return out


def pstream(seed: int, pixel: int, sample: int, n: int) -> np.ndarray:
    out = np.zeros(n, np.uint64)
    lib().orc_pstream(seed, pixel, sample, n, out.ctypes.data)
    return out


# orc_ray (rt_ray's layout: the product binding's RAY records pass as they are) and orc_hit
ORC_RAY = np.dtype([("o", "<f8", (3,)), ("d", "<f8", (3,)), ("time", "<f8"), ("t_min", "<f8"), ("t_max", "<f8"),
                    ("key_pixel", "<u4"), ("key_sample", "<u4")])
ORC_HIT = np.dtype([("t", "<f8"), ("p", "<f8", (3,)), ("n", "<f8", (3,)), ("albedo", "<f8", (3,)), ("hit", "<i4"),
                    ("front_face", "<i4"), ("mat", "<i4"), ("top", "<i4")])
assert ORC_RAY.itemsize == 80 and ORC_HIT.itemsize == 96


def _ray_records(rays) -> np.ndarray:
    rays = np.ascontiguousarray(rays)
    assert rays.dtype.itemsize == 80 and rays.dtype.names == ORC_RAY.names and rays.ndim == 1, rays.dtype
    return rays


def scene_hit(scene_id: int, rays, seed: int = 1, bounce: int = 0, scene_seed: int = 1) -> np.ndarray:
    """orc_scene_hit: the ORC_HIT records of hit_hittables over a built-in scene for caller rays."""
    rays = _ray_records(rays)
    img = earth_texture() if scene_id in (3, 7) else np.zeros((1, 1, 3), np.uint8)
    out = np.zeros(rays.shape[0], dtype=ORC_HIT)
    rc = lib().orc_scene_hit(scene_id, scene_seed, img.ctypes.data, img.shape[1], img.shape[0], seed, bounce,
                             rays.shape[0], rays.ctypes.data, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"orc_scene_hit failed: {rc}")
    return out


class OracleWorld:
    """A custom world in the oracle (orc_world_*), built with the calls of the product's
    rtiow_amd.World; TwinWorld below issues every call to both."""

    def __init__(self, scene_seed: int = 1):
        l = lib()
        self.h = ctypes.c_void_p()
        if l.orc_world_create(ctypes.c_uint64(scene_seed), ctypes.byref(self.h)) != 0:
            raise RuntimeError("orc_world_create")

    def close(self):
        if self.h:
            lib().orc_world_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        self.close()

    @staticmethod
    def _d3(v):
        return (ctypes.c_double * 3)(*[float(x) for x in v])

    def _id(self, rc):
        if rc < 0:
            raise RuntimeError(f"oracle world call failed: {rc}")
        return rc

    def solid(self, r, g, b): return self._id(lib().orc_world_texture(self.h, 0, self._d3((r, g, b)), self._d3((0, 0, 0)), 0.0))
    def checker(self, even, odd): return self._id(lib().orc_world_texture(self.h, 1, self._d3(even), self._d3(odd), 0.0))
    def noise(self, scale): return self._id(lib().orc_world_texture(self.h, 2, self._d3((0, 0, 0)), self._d3((0, 0, 0)), scale))

    def image(self, rgb):
        """Texture::Image over an (h, w, 3) uint8 array; the oracle copies the texels."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        assert rgb.ndim == 3 and rgb.shape[2] == 3, rgb.shape
        return self._id(lib().orc_world_texture_image(self.h, rgb.ctypes.data, rgb.shape[1], rgb.shape[0]))

    def _mat(self, kind, tex=0, albedo=(0, 0, 0), fuzz=0.0, ir=0.0):
        return self._id(lib().orc_world_material(self.h, kind, tex, self._d3(albedo), fuzz, ir))
    def lambertian(self, tex): return self._mat(0, tex)
    def metal(self, albedo, fuzz): return self._mat(1, albedo=albedo, fuzz=fuzz)
    def dielectric(self, ir): return self._mat(2, ir=ir)
    def diffuse_light(self, tex): return self._mat(3, tex)
    def isotropic(self, tex): return self._mat(4, tex)
    def sphere(self, mat, c, r): return self._id(lib().orc_world_sphere(self.h, mat, self._d3(c), r))
    def moving_sphere(self, mat, c0, c1, t0, t1, r):
        return self._id(lib().orc_world_moving_sphere(self.h, mat, self._d3(c0), self._d3(c1), t0, t1, r))
    def xy_rect(self, mat, a0, a1, b0, b1, k): return self._id(lib().orc_world_rect(self.h, 0, mat, a0, a1, b0, b1, k))
    def xz_rect(self, mat, a0, a1, b0, b1, k): return self._id(lib().orc_world_rect(self.h, 1, mat, a0, a1, b0, b1, k))
    def yz_rect(self, mat, a0, a1, b0, b1, k): return self._id(lib().orc_world_rect(self.h, 2, mat, a0, a1, b0, b1, k))
    def box(self, mn, mx, mat): return self._id(lib().orc_world_box(self.h, self._d3(mn), self._d3(mx), mat))
    def translate(self, child, off): return self._id(lib().orc_world_translate(self.h, child, self._d3(off)))
    def rotate_y(self, child, angle): return self._id(lib().orc_world_rotate_y(self.h, child, angle))
    def constant_medium(self, b, density, phase): return self._id(lib().orc_world_constant_medium(self.h, b, density, phase))

    def bvh(self, ids, t0=0.0, t1=1.0):
        arr = (ctypes.c_int * len(ids))(*ids)
        return self._id(lib().orc_world_bvh(self.h, arr, len(ids), t0, t1))

    def push(self, hid):
        self._id(lib().orc_world_push(self.h, hid))

    def hit(self, rays, seed=1, bounce=0) -> np.ndarray:
        """orc_world_hit: the ORC_HIT records of hit_hittables over this world for caller rays."""
        rays = _ray_records(rays)
        out = np.zeros(rays.shape[0], dtype=ORC_HIT)
        rc = lib().orc_world_hit(self.h, seed, bounce, rays.shape[0], rays.ctypes.data, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"orc_world_hit failed: {rc}")
        return out

    def render(self, cam24, bg, width, height, spp, max_depth=50, render_seed=1, row_begin=0, row_stride=1,
               spp_chunk=0, threads=0):
        if threads <= 0:
            threads = min(8, os.cpu_count() or 1)
        if spp_chunk <= 0:
            spp_chunk = min(16, max(1, (spp + 15) // 16))
        n_rows = 0 if row_begin >= height else (height - row_begin + row_stride - 1) // row_stride
        p = Params(-1, 0, render_seed, width, height, spp, max_depth, spp_chunk, row_begin, row_stride, threads,
                   SPLIT_ROWS, None, 0, 0)
        out = np.zeros((n_rows, width, 3), dtype=np.float64)
        cam = np.ascontiguousarray(cam24, dtype=np.float64)
        rc = lib().orc_world_render(self.h, ctypes.byref(p), cam.ctypes.data, self._d3(bg), out.ctypes.data, None)
        if rc != 0:
            raise RuntimeError(f"orc_world_render failed: {rc}")
        return out


class TwinWorld:
    """One custom world built in the product (rtiow_amd.World) and in the oracle by the same
    constructor calls. Texture ids and material handles agree on both sides (checked);
    hittable ids are each side's own (the product's arena also holds a BVH's inner nodes),
    so hittable arguments are translated through a product-id -> oracle-id table."""

    HITTABLE_ARGS = {"translate": (0,), "rotate_y": (0,), "constant_medium": (0,), "push": (0,)}
    SAME_IDS = {"solid", "checker", "noise", "image", "lambertian", "metal", "dielectric", "diffuse_light", "isotropic"}

    def __init__(self, rt, scene_seed: int = 1):
        self.product = rt.World(scene_seed)
        self.oracle = OracleWorld(scene_seed)
        self.to_oracle = {}

    def bvh(self, ids, t0=0.0, t1=1.0):
        a = self.product.bvh(ids, t0, t1)
        self.to_oracle[a] = self.oracle.bvh([self.to_oracle[i] for i in ids], t0, t1)
        return a

    def __getattr__(self, name):
        def call(*args):
            a = getattr(self.product, name)(*args)
            oargs = list(args)
            for i in self.HITTABLE_ARGS.get(name, ()):
                oargs[i] = self.to_oracle[args[i]]
            b = getattr(self.oracle, name)(*oargs)
            if name in self.SAME_IDS:
                assert a == b, (name, a, b)
            elif isinstance(a, int) and name != "push":
                self.to_oracle[a] = b
            return a
        return call
