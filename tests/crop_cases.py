"""Shared by the YOLO-Crop+UNet tests (helper module, like tests/buffer_guard.py): the box set, thin wrappers of the host twins of
include/openglottal_hip_crops.h, and the host composition the device engine is compared with."""
import ctypes as C

import numpy as np

from openglottal_amd import geometry
from openglottal_amd._lib import check, lib

H, W, SIZE = 80, 96, 32

# (x1, y1, x2, y2) inside an 80 x 96 frame, usable at size 32
USABLE = [
    (0, 0, W, H),          # the whole frame (downscale)
    (0, 10, 40, 50),       # touching the left border
    (50, 0, 90, 30),       # the top
    (60, 20, W, 70),       # the right
    (10, 40, 70, H),       # the bottom
    (20, 5, 21, 65),       # 1 pixel wide, long side 60 < 2 * size: round(32 / 60) = 1
    (5, 30, 55, 31),       # 1 pixel tall
    (30, 5, 50, 75),       # taller than wide
    (5, 30, 90, 50),       # wider than tall
    (40, 40, 50, 52),      # smaller than the tile (upscale)
    (10, 10, 42, 30),      # long side == size: the identity shortcut of the projection on that axis
    (7, 3, 40, 67),        # 33 x 64: the short side scales to 16.5 -> 16 (half to even)
]
SLIVER = (3, 0, 4, H)      # 1 x 80: round(32 / 80) = 0
EMPTY = (5, 5, 5, 20)
UNUSABLE = [(-1, -1, -1, -1), EMPTY, SLIVER, (50, 50, 120, 70), (10, 60, 30, 81), (0, 0, 0, 0)]


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def geometry_host(h, w, size):
    g = np.full(4, -7, np.int32)
    rc = lib().og_crop_geometry_host(h, w, size, g.ctypes.data)
    return rc, tuple(int(v) for v in g)


def tile_host(frame, box, size):
    frame = np.ascontiguousarray(frame, dtype=np.uint8)
    ch = 3 if frame.ndim == 3 else 1
    tile = np.full((size, size), 0x5A, np.uint8)
    b = i32(box)
    check(lib().og_crop_tile_host(frame.ctypes.data, frame.shape[0], frame.shape[1], ch, b.ctypes.data, size, tile.ctypes.data), "og_crop_tile_host")
    return tile


def project_host(tile_mask, box, h, w, want_mask=True):
    tile_mask = np.ascontiguousarray(tile_mask, dtype=np.uint8)
    mask = np.full((h, w), 0x5A, np.uint8) if want_mask else None
    area = np.full(1, -7, np.int32)
    b = i32(box)
    check(lib().og_crop_project_host(tile_mask.ctypes.data, tile_mask.shape[0], b.ctypes.data, h, w, None if mask is None else mask.ctypes.data,
                                     area.ctypes.data), "og_crop_project_host")
    return mask, int(area[0])


def numpy_tile(gray, box, size):
    """infer.py:232-237 in numpy (geometry.py)."""
    x1, y1, x2, y2 = box
    return geometry.letterbox_with_info(gray[y1:y2, x1:x2], size, value=0)


def numpy_project(tile_mask, box, geom, h, w):
    """infer.py:239-246 in numpy (geometry.py): (full-frame mask, area)."""
    x1, y1, x2, y2 = box
    m = geometry.unletterbox(tile_mask, *geom, y2 - y1, x2 - x1)
    full = np.zeros((h, w), np.uint8)
    full[y1:y2, x1:x2] = m
    return full, int(np.sum(m > 0))


def host_composition(model, frames, boxes, size, threshold=0.5):
    """og_crop_tile_host tiles -> model.segment -> og_crop_project_host, frame by frame list in, (mask [B,H,W], area [B]) out."""
    B = len(frames)
    h, w = frames[0].shape[:2]
    tiles = np.stack([tile_host(f, b, size) for f, b in zip(frames, boxes)])
    tm, _, _ = model.segment(tiles, threshold=threshold, want_area=False)
    mask, area = np.empty((B, h, w), np.uint8), np.empty(B, np.int32)
    for i in range(B):
        mask[i], area[i] = project_host(tm[i], boxes[i], h, w)
    return mask, area


def plan_crops(features, B, h, w, channels, boxes, size, lanes, options=""):
    """og_unet_plan_crops -> (list of records, arena bytes)."""
    feats = (C.c_int * len(features))(*features)
    out = C.create_string_buffer(1 << 20)
    arena = C.c_longlong(-1)
    bx = i32(boxes)
    n = lib().og_unet_plan_crops(feats, len(features), B, h, w, channels, bx.ctypes.data, size, lanes, options.encode(), out, len(out), C.byref(arena))
    assert n >= 0, (n, lib().og_last_error())
    recs = []
    for line in out.value.decode().splitlines():
        f = line.split("|")
        writes = {} if f[8] == "-" else {k: int(v) for k, v in (kv.split("=") for kv in f[8].split(";"))}
        recs.append({"kernel": f[0], "grid": tuple(int(v) for v in f[1:4]), "block": int(f[4]), "lds": int(f[5]), "workspace": int(f[6]),
                     "counters": int(f[7]), "writes": writes})
    assert len(recs) == n
    return recs, int(arena.value)
