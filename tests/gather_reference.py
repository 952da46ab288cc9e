"""The gather path's layout restated in plain numpy (no library call): what rt_render_gather's
ranks send, where it lands on rank 0 and how the frame is read back out of it. The statement
under test is csrc/comm_layout.hpp (slab geometry, status scan), rt_tiles_in_shard,
rt_tiles_assemble_host and the reorder kernel (rt_tiles_assemble); this one is written from
include/rt/rt_abi.h's description of the tile shard and of rt_render_gather alone.

A frame's 8x8 tiles are numbered in raster order, t = ty * tiles_x + tx; edge tiles are cut by
the frame. A tile order maps a position to a raster tile (None: the identity). Rank r of `world`
holds the positions r, r + world, ...: n_r of them. Its slab is 8 rows x 8 n_r columns x 3
elements, its m-th tile in columns 8 m .. 8 m + 7 (a cut tile's columns and rows outside the
frame hold no image data), padded to rank 0's size (n_max = n_0 tiles) and followed by an
8-byte trailer: an int32 status (0, or minus the error code of the rank's render) and an int32 0.
"""
import numpy as np

TRAILER_BYTES = 8


def n_tiles(width, height):
    return ((width + 7) // 8) * ((height + 7) // 8)


def tiles_in_shard(width, height, rank, world):
    """Tile positions rank, rank + world, ... below the frame's tile count."""
    return len(range(rank, n_tiles(width, height), world))


def slab_geometry(width, height, world, esz):
    """The slab layout at one frame, world size and element size, under the names
    tests/comm_layout_dump.cpp prints."""
    n_max = tiles_in_shard(width, height, 0, world)
    slab_elems = 8 * 8 * 3 * n_max
    slab_bytes = slab_elems * esz + TRAILER_BYTES
    assert slab_bytes % esz == 0
    return {"world": world, "esz": esz, "n_max": n_max, "slab_elems": slab_elems, "slab_bytes": slab_bytes,
            "status_off": slab_elems * esz, "stride_elems": slab_bytes // esz, "gathered_bytes": world * slab_bytes,
            "trailer_bytes": TRAILER_BYTES,
            "n_mine": [tiles_in_shard(width, height, r, world) for r in range(world)],
            "status_at": [r * slab_bytes + slab_elems * esz for r in range(world)]}


def _dtype(esz):
    return {4: np.float32, 8: np.float64}[esz]


def statuses(gathered, width, height, world, esz):
    """The `world` status words of a gathered byte buffer."""
    g = slab_geometry(width, height, world, esz)
    b = np.ascontiguousarray(gathered, dtype=np.uint8).reshape(-1)
    assert b.size == g["gathered_bytes"]
    return [int(np.frombuffer(b[at:at + 4].tobytes(), dtype=np.int32)[0]) for at in g["status_at"]]


def status_scan(status):
    """(failed ranks, the first of them or -1, the RT_ERR_* code (negative) its render returned or 0)."""
    bad = [r for r, s in enumerate(status) if s != 0]
    return {"failed": len(bad), "first": bad[0] if bad else -1, "first_rc": -status[bad[0]] if bad else 0}


def reassemble(gathered, width, height, world, esz, order=None, fill=0.0):
    """A world x slab_bytes byte buffer -> the height x width x 3 frame, under an optional tile
    order; pixels no slab covers (there are none for a permutation) keep `fill`."""
    g = slab_geometry(width, height, world, esz)
    b = np.ascontiguousarray(gathered, dtype=np.uint8).reshape(-1)
    assert b.size == g["gathered_bytes"]
    tiles_x = (width + 7) // 8
    total = n_tiles(width, height)
    if order is not None:
        order = [int(t) for t in order]
        assert sorted(order) == list(range(total))
    frame = np.full((height, width, 3), fill, dtype=_dtype(esz))
    for r in range(world):
        n_r = g["n_mine"][r]
        base = r * g["slab_bytes"]
        slab = np.frombuffer(b[base:base + 192 * n_r * esz].tobytes(), dtype=_dtype(esz)).reshape(8, 8 * n_r, 3)
        for m in range(n_r):
            pos = r + m * world
            t = pos if order is None else order[pos]
            y0, x0 = (t // tiles_x) * 8, (t % tiles_x) * 8
            h, w = min(8, height - y0), min(8, width - x0)
            frame[y0:y0 + h, x0:x0 + w] = slab[:h, 8 * m:8 * m + w]
    return frame


def scatter(frame, world, order=None, pad_byte=0xFF, status=None):
    """The inverse, for CPU tests: the gathered byte buffer that holds `frame`, everything the
    frame does not define (cut tiles' outside pixels, padding, and the trailers unless `status`
    gives them) set to pad_byte."""
    height, width = frame.shape[:2]
    esz = frame.dtype.itemsize
    g = slab_geometry(width, height, world, esz)
    tiles_x = (width + 7) // 8
    b = np.full(g["gathered_bytes"], pad_byte, dtype=np.uint8)
    for r in range(world):
        n_r = g["n_mine"][r]
        slab = np.frombuffer(bytes([pad_byte]) * (192 * n_r * esz), dtype=frame.dtype).reshape(8, 8 * n_r, 3).copy()
        for m in range(n_r):
            pos = r + m * world
            t = pos if order is None else int(order[pos])
            y0, x0 = (t // tiles_x) * 8, (t % tiles_x) * 8
            h, w = min(8, height - y0), min(8, width - x0)
            slab[:h, 8 * m:8 * m + w] = frame[y0:y0 + h, x0:x0 + w]
        base = r * g["slab_bytes"]
        b[base:base + slab.nbytes] = np.frombuffer(slab.tobytes(), dtype=np.uint8)
        if status is not None:
            b[g["status_at"][r]:g["status_at"][r] + 8] = np.frombuffer(
                np.array([status[r], 0], dtype=np.int32).tobytes(), dtype=np.uint8)
    return b
