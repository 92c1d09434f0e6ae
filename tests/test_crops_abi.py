"""The rules tests/test_host_logic.py and tests/test_buffer_guard.py hold include/openglottal_hip.h to, on the second header
include/openglottal_hip_crops.h: every function it declares is exported and bound (`_lib.CROP_PROTOTYPES`) and vice versa; every
function with a caller's buffer is in the extents matrix of tests/test_gpu_crop_extents.py, host only (and then held to its extents
here) or exempt for a stated reason; misaligned int32 pointers are refused before anything is written.  No GPU."""
import os
import re

import numpy as np

import buffer_guard as G
import crop_cases as K
from openglottal_amd import _lib
from openglottal_amd._lib import lib
from openglottal_amd.utils import bgr_to_gray_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL = -1

EXEMPT = {
    "og_unet_plan_crops": "plan recorder: host text bounded by cap (tests/test_crop_plan.py)",
}
HOST_ONLY = {"og_crop_geometry_host", "og_crop_tile_host", "og_crop_project_host"}


def _declarations(header):
    """name -> parameter list of every function a header declares (comments stripped)."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_function_of_the_crops_header_is_exported_and_bound_and_vice_versa():
    declared = set(_declarations("openglottal_hip_crops.h"))
    assert len(declared) == 7 and "og_unet_stream_crops_u8" in declared
    l = lib()
    for name in sorted(declared):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        assert getattr(l, name).argtypes == _lib.CROP_PROTOTYPES[name][1]        # lib() bound it
    assert declared == set(_lib.CROP_PROTOTYPES), declared ^ set(_lib.CROP_PROTOTYPES)
    assert not (set(_lib.CROP_PROTOTYPES) & set(_lib.PROTOTYPES))
    for name, (_, args) in _lib.CROP_PROTOTYPES.items():
        assert len(args) == len(_declarations("openglottal_hip_crops.h")[name]), name


def test_the_main_header_still_equals_prototypes():
    assert set(_declarations("openglottal_hip.h")) == set(_lib.PROTOTYPES)
    assert '#include "openglottal_hip.h"' in open(os.path.join(ROOT, "include", "openglottal_hip_crops.h")).read()


def test_lib_fails_loudly_on_a_missing_crop_symbol(monkeypatch):
    import ctypes as C

    import pytest

    real = lib()

    class Without:
        def __getattr__(self, name):
            if name == "og_unet_stream_crops_u8":
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(C, "CDLL", lambda path: Without())
    with pytest.raises(AttributeError, match="og_unet_stream_crops_u8"):
        _lib.lib()
    monkeypatch.setattr(_lib, "_lib", real)


def test_every_crop_entry_with_a_caller_buffer_is_in_the_matrix_host_only_or_exempt():
    import test_gpu_crop_extents as M

    fns = {}
    for name, params in _declarations("openglottal_hip_crops.h").items():
        bufs = [p for p in params if "*" in p and not re.match(r"og_unet\s*\*\s*h$", p) and not re.match(r"const\s+char\s*\*", p)]
        if bufs:
            fns[name] = bufs
    assert len(fns) == 7
    assert not (set(M.CROP_MATRIX) & set(EXEMPT)) and not (HOST_ONLY & set(EXEMPT)) and not (HOST_ONLY & set(M.CROP_MATRIX))
    for name in fns:
        assert name in M.CROP_MATRIX or name in HOST_ONLY or name in EXEMPT, f"{name}{fns[name]}: not covered and not exempt"
    for name in list(M.CROP_MATRIX) + list(EXEMPT) + list(HOST_ONLY):
        assert name in fns, f"{name}: listed, but the header has no such function with a caller's buffer"
    for name, test in M.CROP_MATRIX.items():
        assert all(callable(getattr(M, t, None)) for t in test.split()), (name, test)


# ── the host-only entries inside guards ──────────────────────────────────────────
def test_crop_geometry_host_extents():
    for h, w, size in ((33, 64, 32), (1, 64, 32), (80, 96, 256), (130, 1, 64)):
        out = G.run_guarded("og_crop_geometry_host", f"{h}x{w}->{size}", lambda p: lib().og_crop_geometry_host(h, w, size, p["geom4"]),
                            {}, {"geom4": 16})
        s = size / max(h, w)
        nh, nw = int(round(h * s)), int(round(w * s))
        assert tuple(out["geom4"].view(np.int32)) == ((size - nh) // 2, (size - nw) // 2, nh, nw)


def test_crop_tile_and_project_host_extents():
    rs = np.random.RandomState(5)
    bgr = rs.randint(0, 256, (K.H, K.W, 3), dtype=np.uint8)
    gray = bgr_to_gray_numpy(bgr)
    for box in K.USABLE + K.UNUSABLE:
        b4 = K.i32(box)
        tiles = []
        for frame, ch in ((gray, 1), (bgr, 3)):
            out = G.run_guarded("og_crop_tile_host", f"box={box} ch={ch}",
                                lambda p: lib().og_crop_tile_host(p["frame"], K.H, K.W, ch, p["box4"], K.SIZE, p["tile"]),
                                {"frame": frame, "box4": b4}, {"tile": K.SIZE * K.SIZE})
            tiles.append(out["tile"])
        assert np.array_equal(tiles[0], tiles[1])
        tm = (rs.randint(0, 2, (K.SIZE, K.SIZE)) * 255).astype(np.uint8)
        got = {}
        for want_mask in (True, False):
            out = G.run_guarded("og_crop_project_host", f"box={box} mask={want_mask}",
                                lambda p: lib().og_crop_project_host(p["tile_mask"], K.SIZE, p["box4"], K.H, K.W, p["mask"], p["area"]),
                                {"tile_mask": tm, "box4": b4}, {"mask": K.H * K.W if want_mask else None, "area": 4})
            got[want_mask] = out
        area = int(got[True]["area"].view(np.int32)[0])
        assert area == int(got[False]["area"].view(np.int32)[0]) == int((got[True]["mask"] > 0).sum())
        assert (box in K.USABLE) or (area == 0 and not tiles[0].any())


def test_misaligned_int32_pointers_are_refused_by_the_host_only_crop_entries():
    buf = G.Region("b", 1 << 16, "host", G.guard_bytes(1 << 16), G.GUARD_FILL)
    a = buf.ptr
    frame, tile, box, area, mask = a, a + 32768, a + 40000, a + 40064, a + 41000      # (all inside the payload; 4-byte aligned)
    good = np.array(K.USABLE[1], np.int32)
    G.view(box, 16)[:] = good.view(np.uint8)
    before = buf.snapshot()
    for off in (1, 2, 3):
        assert lib().og_crop_geometry_host(33, 64, 32, a + off) == OG_EINVAL
        assert lib().og_crop_tile_host(frame, K.H, K.W, 1, box + off, K.SIZE, tile) == OG_EINVAL
        assert lib().og_crop_project_host(tile, K.SIZE, box + off, K.H, K.W, mask, area) == OG_EINVAL
        assert lib().og_crop_project_host(tile, K.SIZE, box, K.H, K.W, mask, area + off) == OG_EINVAL
    assert np.array_equal(buf.snapshot(), before)          # nothing was written by any refused call
    assert lib().og_crop_tile_host(frame + 1, K.H, K.W, 1, box, K.SIZE, tile + 3) == 0        # u8 buffers: any address
    assert lib().og_crop_project_host(tile + 3, K.SIZE, box, K.H, K.W, mask + 1, area) == 0


def test_the_plan_entry_refuses_a_misaligned_boxes_pointer():
    import ctypes as C

    feats = (C.c_int * 4)(4, 8, 16, 32)
    raw = np.zeros(64, np.uint8)          # two all-zero rows: empty boxes
    out = C.create_string_buffer(4096)
    base = raw.ctypes.data + (-raw.ctypes.data) % 8
    assert lib().og_unet_plan_crops(feats, 4, 2, K.H, K.W, 1, base + 2, K.SIZE, 1, b"", out, 4096, None) == OG_EINVAL
    assert lib().og_unet_plan_crops(feats, 4, 2, K.H, K.W, 1, base, K.SIZE, 1, b"", out, 4096, None) == 0
