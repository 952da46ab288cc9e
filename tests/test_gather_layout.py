"""The gather path's layout on the CPU: csrc/comm_layout.hpp (the slab geometry and status scan
rt_render_gather runs on, printed by tests/comm_layout_dump.cpp), rt_tiles_in_shard and
rt_tiles_assemble_host, each held to tests/gather_reference.py's plain numpy restatement.

comm_layout_dump links launch_plan.cpp and nothing from HIP. It is built twice, plain and as its
own program with ASan and UBSan (the program itself is instrumented, so nothing is preloaded);
both must print the same. Every comparison is equality: integers, or frames bit for bit.

The shapes are the smallest with each edge: (160, 90) a cut last tile row, (40, 24) 15 tiles
(at world 8 ranks hold 2 and 1), (67, 5) ragged in both axes, (9, 7) 2 tiles (at world 3 and 8
most ranks hold none). tests/test_gpu_gather_layout.py runs the same layout on the GPU.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from tests import gather_reference as gr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "rust-ray-tracing-in-a-weekend_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
BASE = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
SOURCES = [os.path.join(REPO, "tests", "comm_layout_dump.cpp"), os.path.join(CSRC, "launch_plan.cpp")]

SHAPES = [(160, 90), (40, 24), (67, 5), (9, 7)]
WORLDS = [1, 2, 3, 8]
ORDERS = ["raster", "reversed", "permuted"]
NO_SCENE, HIP = 6, 2   # status words: minus RT_ERR_NO_SCENE, minus RT_ERR_HIP


def tile_order(kind, n, seed=1234):
    """raster -> None; reversed; a seeded permutation."""
    if kind == "raster":
        return None
    if kind == "reversed":
        return np.arange(n, dtype=np.uint32)[::-1].copy()
    return np.random.default_rng(seed).permutation(n).astype(np.uint32)


def status_vectors(world):
    """No failure; rank 0 alone; the last rank alone; two ranks (the last two; world 1 has one)."""
    none = [0] * world
    first = [NO_SCENE] + [0] * (world - 1)
    last = [0] * (world - 1) + [HIP]
    two = [0] * max(world - 2, 0) + [HIP, NO_SCENE][-min(world, 2):]
    return [none, first, last, two]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """dump(W, H, world, esz, status) -> comm_layout_dump's JSON, equal from both builds."""
    d = tmp_path_factory.mktemp("comm_layout")
    exes = []
    for name, flags in (("plain", []), ("san", SAN)):
        exe = str(d / ("comm_layout_dump_" + name))
        b = subprocess.run([CLANG, *BASE, *flags, "-I" + os.path.join(REPO, "include"), "-I" + CSRC, *SOURCES, "-o", exe],
                           capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-4000:]
        exes.append(exe)

    def run(width, height, world, esz, status=()):
        outs = []
        for exe in exes:
            env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1",
                       UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
            r = subprocess.run([exe, str(width), str(height), str(world), str(esz), *[str(s) for s in status]],
                               capture_output=True, text=True, env=env, timeout=60)
            report = r.stdout + r.stderr
            assert "Sanitizer" not in report and "runtime error" not in report, report[-4000:]
            assert r.returncode == 0, report[-4000:]
            outs.append(r.stdout)
        assert outs[0] == outs[1]
        return json.loads(outs[0])
    return run


@pytest.mark.parametrize("shape", SHAPES)
def test_layout_and_status_scan_equal_the_reference(dump, shape):
    """Every (shape, world, element size): the geometry, and the scan of each status vector."""
    width, height = shape
    for world in WORLDS:
        for esz in (4, 8):
            want = gr.slab_geometry(width, height, world, esz)
            for status in status_vectors(world):
                got = dump(width, height, world, esz, status)
                assert {k: got[k] for k in want} == want, (shape, world, esz)
                scan = gr.status_scan(status)
                assert {k: got[k] for k in scan} == scan, (shape, world, esz, status)
                assert got["status_of"] == list(range(9))   # rc 0, -1, ... -8 -> 0, 1, ... 8
            # the figures the issue of this layout quotes: the trailer rides in the kernel's stride
            assert want["stride_elems"] == 192 * want["n_max"] + (1 if esz == 8 else 2)
            assert want["status_at"][-1] + 8 == want["gathered_bytes"]


def test_reference_geometry_at_the_shapes_edges():
    """What each shape is there for, from the reference alone."""
    assert gr.n_tiles(160, 90) == 20 * 12 and 90 % 8 == 2
    assert gr.slab_geometry(40, 24, 8, 8)["n_mine"] == [2, 2, 2, 2, 2, 2, 2, 1]
    assert gr.n_tiles(67, 5) == 9 and 67 % 8 == 3
    assert gr.slab_geometry(9, 7, 3, 4)["n_mine"] == [1, 1, 0]
    assert gr.slab_geometry(9, 7, 8, 4)["n_mine"] == [1, 1, 0, 0, 0, 0, 0, 0]
    st = [0, 0, HIP, 0, NO_SCENE]
    assert gr.status_scan(st) == {"failed": 2, "first": 2, "first_rc": -HIP}   # RT_ERR_HIP itself


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    path = os.path.join(ge.PKG, "lib", "librtiow_amd.so")
    if not os.path.exists(path):
        ge.build_library()
    return ge.import_binding().load_library()


def random_frame(width, height, dtype, seed):
    """Finite values with random mantissas: a NaN in a result can only come from padding."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((height, width, 3)) * 1e3).astype(dtype)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("world", WORLDS)
def test_host_assembly_equals_the_reference(lib, shape, world):
    """rt_tiles_in_shard and rt_tiles_assemble_host on the trailer-strided layout the library
    gathers: padding, cut tiles' outside pixels and trailers are NaN bytes, none may reach the frame."""
    width, height = shape
    total = gr.n_tiles(width, height)
    for r in range(world + 2):   # (ranks past the world too: the count is of positions r, r + world, ...)
        assert lib.rt_tiles_in_shard(width, height, r, world) == gr.tiles_in_shard(width, height, r, world)
    for dtype in (np.float32, np.float64):
        esz = np.dtype(dtype).itemsize
        g = gr.slab_geometry(width, height, world, esz)
        for kind in ORDERS:
            order = tile_order(kind, total)
            frame = random_frame(width, height, dtype, seed=world * 100 + esz)
            gathered = gr.scatter(frame, world, order, pad_byte=0xFF)
            assert gr.statuses(gathered, width, height, world, esz) == [-1] * world   # 0xFF trailers
            ref = gr.reassemble(gathered, width, height, world, esz, order, fill=np.nan)
            assert np.array_equal(ref, frame)   # (no NaN: equality would fail on one)
            got = np.full((height, width, 3), np.nan, dtype=dtype)
            before = gathered.copy()
            rc = lib.rt_tiles_assemble_host(gathered.ctypes.data, ctypes.c_int64(g["stride_elems"]), world, width, height,
                                            esz, None if order is None else order.ctypes.data, got.ctypes.data)
            assert rc == 0, (shape, world, esz, kind)
            assert not np.isnan(got).any(), (shape, world, esz, kind)
            assert np.array_equal(got.view(np.uint8), frame.view(np.uint8)), (shape, world, esz, kind)
            assert np.array_equal(gathered, before)
            # the untrailed stride (192 n_max) reads rank r >= 1 at another place: the layouts differ
            if world > 1 and g["n_mine"][1] > 0:
                bad = np.full((height, width, 3), np.nan, dtype=dtype)
                rc = lib.rt_tiles_assemble_host(gathered.ctypes.data, ctypes.c_int64(g["slab_elems"]), world, width,
                                                height, esz, None if order is None else order.ctypes.data,
                                                bad.ctypes.data)
                assert rc == 0 and not np.array_equal(bad.view(np.uint8), frame.view(np.uint8))
