"""Reference side of the feature-buffer tests (test_gpu_features.py, test_gpu_denoise_guided.py).
Nothing here calls rt_render_features.

LightTwin. A world built in the product as written and in the oracle with every material replaced
by a diffuse_light over the colour rt_render_features' albedo names for it (include/rt/rt_abi.h):
lambertian(tex), isotropic(tex) -> light(tex); metal(albedo) -> light(solid(albedo)); dielectric ->
light(solid(1, 1, 1)); a light stays. The oracle's ray_color at max_depth = 1 returns the first
hit's emitted colour, or the background on a miss, so OracleWorld.render(..., max_depth=1,
spp_chunk=c) of the twin is the albedo buffer: the same primary rays (the medium's keyed draw
included) and the same chunked sum. The extra solid textures shift the oracle's texture ids, hence
the product -> oracle texture and material tables; solid textures and materials draw nothing from
the construction stream, so Perlin tables and BVH axes stay those of the plain twin.

first_hit. A numpy restatement of the first hit for worlds of top-level static spheres and
axis-aligned rects under a camera of aperture 0: per (pixel, sample) the ray from the path stream's
first two draws (oracle_binding.pstream, mapped by orc_eval fn 10), the oracle's sphere and rect
formulas (oracle.c sphere_hit, rect_hit) over the list in order with t in (0.001, closest so far).
"""
import numpy as np

from tests import oracle_binding as ob


class LightTwin:
    """tests/oracle_binding.py TwinWorld's interface; the oracle side holds lights only."""

    MAT_ARG = {"sphere": 0, "moving_sphere": 0, "xy_rect": 0, "xz_rect": 0, "yz_rect": 0, "box": 2, "constant_medium": 2}
    HITTABLE_ARGS = ob.TwinWorld.HITTABLE_ARGS

    def __init__(self, rt, scene_seed: int = 1):
        self.product = rt.World(scene_seed)
        self.oracle = ob.OracleWorld(scene_seed)
        self.to_oracle = {}
        self.tex = {}
        self.mat = {}

    # textures: the same call on both sides
    def _texture(self, name, *args):
        a = getattr(self.product, name)(*args)
        self.tex[a] = getattr(self.oracle, name)(*args)
        return a

    def solid(self, r, g, b): return self._texture("solid", r, g, b)
    def checker(self, even, odd): return self._texture("checker", even, odd)
    def noise(self, scale): return self._texture("noise", scale)

    # materials: the product's as written, the oracle's a light over the albedo's colour
    def _light(self, a, otex):
        self.mat[a] = self.oracle.diffuse_light(otex)
        return a

    def lambertian(self, tex): return self._light(self.product.lambertian(tex), self.tex[tex])
    def isotropic(self, tex): return self._light(self.product.isotropic(tex), self.tex[tex])
    def diffuse_light(self, tex): return self._light(self.product.diffuse_light(tex), self.tex[tex])
    def metal(self, albedo, fuzz): return self._light(self.product.metal(albedo, fuzz), self.oracle.solid(*albedo))
    def dielectric(self, ir): return self._light(self.product.dielectric(ir), self.oracle.solid(1.0, 1.0, 1.0))

    def bvh(self, ids, t0=0.0, t1=1.0):
        a = self.product.bvh(ids, t0, t1)
        self.to_oracle[a] = self.oracle.bvh([self.to_oracle[i] for i in ids], t0, t1)
        return a

    def __getattr__(self, name):
        if name.startswith("_") or name in ("product", "oracle", "to_oracle", "tex", "mat"):
            raise AttributeError(name)

        def call(*args):
            a = getattr(self.product, name)(*args)
            oargs = list(args)
            for i in self.HITTABLE_ARGS.get(name, ()):
                oargs[i] = self.to_oracle[args[i]]
            if name in self.MAT_ARG:
                oargs[self.MAT_ARG[name]] = self.mat[args[self.MAT_ARG[name]]]
            b = getattr(self.oracle, name)(*oargs)
            if isinstance(a, int) and name != "push":
                self.to_oracle[a] = b
            return a
        return call


def cam24(cam) -> np.ndarray:
    v = []
    for f in ("origin", "lower_left_corner", "horizontal", "vertical", "u", "v", "w"):
        v += list(getattr(cam, f))
    return np.array(v + [cam.lens_radius, cam.time0, cam.time1])


# ---- the numpy first-hit reference -------------------------------------------------------------------
# a primitive: ("sphere", (cx, cy, cz), radius, (r, g, b)) or
#              ("rect", axis, a0, a1, b0, b1, k, (r, g, b))   axis 0: XY, 1: XZ, 2: YZ (oracle.c rect_hit)
# the colour is the albedo the material's definition names (solid textures only)
T_MIN = 0.001


def build_simple(rt, prims, materials, scene_seed: int = 1):
    """The product world of a primitive list; materials[i] = ("lambertian" | "metal" | "dielectric" |
    "light") of prims[i], built over a solid texture of the primitive's colour."""
    w = rt.World(scene_seed)
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


def first_hit(prims, cam, bg, W, H, spp, seed: int = 1):
    """(albedo (H, W, 3), normal (H, W, 3), depth (H, W), hits (H, W) = samples that hit) means over spp
    samples. cam: the binding's Camera, lens_radius 0."""
    assert cam.lens_radius == 0.0
    origin, ll, hor, ver = (np.array(list(getattr(cam, f))) for f in ("origin", "lower_left_corner", "horizontal", "vertical"))
    ys, xs = np.mgrid[0:H, 0:W]
    albedo = np.zeros((H, W, 3))
    normal = np.zeros((H, W, 3))
    depth = np.zeros((H, W))
    hits = np.zeros((H, W), dtype=np.int64)
    for s in range(spp):
        bits = np.array([ob.pstream(seed, y * W + x, s, 2) for y in range(H) for x in range(W)], dtype=np.uint64)
        d = ob.evaluate(10, bits.reshape(-1).view(np.float64)).reshape(H, W, 2)
        u = (xs + d[..., 0]) / (W - 1)
        v = (ys + d[..., 1]) / (H - 1)
        dirn = ll + u[..., None] * hor + v[..., None] * ver - origin
        best_t = np.full((H, W), np.inf)
        best_n = np.zeros((H, W, 3))
        best_c = np.zeros((H, W, 3))
        with np.errstate(all="ignore"):
            for prim in prims:
                if prim[0] == "sphere":
                    c, r = np.array(prim[1], dtype=np.float64), float(prim[2])
                    oc = origin - c
                    a = (dirn * dirn).sum(-1)
                    half_b = (oc * dirn).sum(-1)
                    cc = (oc * oc).sum() - r * r
                    disc = half_b * half_b - a * cc
                    sq = np.sqrt(np.where(disc >= 0, disc, 0.0))
                    t0, t1 = (-half_b - sq) / a, (-half_b + sq) / a
                    ok0 = ~((t0 < T_MIN) | (best_t < t0))
                    ok1 = ~((t1 < T_MIN) | (best_t < t1))
                    t = np.where(ok0, t0, t1)
                    hit = (disc >= 0) & (ok0 | ok1)
                    p = origin + t[..., None] * dirn
                    n = (p - c) / r
                else:
                    _, axis, a0, a1, b0, b1, k, _ = prim
                    ka, aa, ba = ((2, 0, 1), (1, 0, 2), (0, 1, 2))[axis]
                    t = (k - origin[ka]) / dirn[..., ka]
                    x = origin[aa] + t * dirn[..., aa]
                    y = origin[ba] + t * dirn[..., ba]
                    hit = ~((t < T_MIN) | (t > best_t)) & ~((x < a0) | (x > a1) | (y < b0) | (y > b1))
                    n = np.zeros((H, W, 3))
                    n[..., ka] = 1.0
                front = (dirn * n).sum(-1) < 0.0
                n = np.where(front[..., None], n, -n)
                best_t = np.where(hit, t, best_t)
                best_n = np.where(hit[..., None], n, best_n)
                best_c = np.where(hit[..., None], np.array(prim[-1], dtype=np.float64), best_c)
        any_hit = np.isfinite(best_t)
        p = origin + np.where(any_hit, best_t, 0.0)[..., None] * dirn
        albedo += np.where(any_hit[..., None], best_c, np.array(bg, dtype=np.float64))
        normal += np.where(any_hit[..., None], best_n, 0.0)
        depth += np.where(any_hit, np.sqrt(((p - origin) ** 2).sum(-1)), 0.0)
        hits += any_hit
    return albedo / spp, normal / spp, depth / spp, hits
