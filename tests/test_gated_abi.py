"""The rules tests/test_classic_abi.py holds the third header to, on the fourth, include/openglottal_hip_gated.h: every function it
declares is exported and bound (`_lib.GATED_PROTOTYPES`) and vice versa; the three older headers and their tables are untouched;
every function with a caller's buffer is in the extents matrix of tests/test_gpu_gated_extents.py, host only (and then held to its
extents here) or exempt for a stated reason; misaligned and null pointers are refused before anything is written; the dry run of
the engine.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import buffer_guard as G
import track_cases as T
from openglottal_amd import _lib, gated
from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL, OG_ESTATE = -1, -2
HEADER = "openglottal_hip_gated.h"

EXEMPT = {
    "og_gated_plan": "plan recorder: host text bounded by cap (test_the_dry_run_* below)",
    "og_gated_set_option": "its only pointer is a NUL-terminated option name",
}
HOST_ONLY = {"og_track_host"}
HANDLE = re.compile(r"(og_gated|og_unet|og_yolo)\s*\*\s*\w+$")


def _declarations(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_function_of_the_gated_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert len(decl) == 13 and "og_gated_stream_u8" in decl
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        assert getattr(l, name).argtypes == _lib.GATED_PROTOTYPES[name][1]
    assert set(decl) == set(_lib.GATED_PROTOTYPES), set(decl) ^ set(_lib.GATED_PROTOTYPES)
    assert not (set(_lib.GATED_PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_lib.CROP_PROTOTYPES) | set(_lib.CLASSIC_PROTOTYPES)))
    for name, (_, args) in _lib.GATED_PROTOTYPES.items():
        n = 0 if decl[name] == ["void"] else len(decl[name])
        assert len(args) == n, name
    required = {"og_track_host", "og_track_boxes_dev", "og_gated_create", "og_gated_destroy", "og_gated_reset", "og_gated_set_params",
                "og_gated_get_state", "og_gated_set_state", "og_gated_stream_u8", "og_gated_stream_frames_u8", "og_gated_plan"}
    assert required <= set(decl)


def test_the_older_headers_still_equal_their_tables_and_are_unchanged():
    assert set(_declarations("openglottal_hip.h")) == set(_lib.PROTOTYPES)
    assert set(_declarations("openglottal_hip_crops.h")) == set(_lib.CROP_PROTOTYPES)
    assert set(_declarations("openglottal_hip_classic.h")) == set(_lib.CLASSIC_PROTOTYPES)
    assert '#include "openglottal_hip.h"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert len(_lib.PROTOTYPES) == 66 and len(_lib.CROP_PROTOTYPES) == 7 and len(_lib.CLASSIC_PROTOTYPES) == 20
    for older in ("openglottal_hip.h", "openglottal_hip_crops.h", "openglottal_hip_classic.h"):
        assert "og_gated" not in open(os.path.join(ROOT, "include", older)).read() and "og_track" not in open(os.path.join(ROOT, "include", older)).read()


def test_every_gated_entry_with_a_caller_buffer_is_in_the_matrix_host_only_or_exempt():
    import test_gpu_gated_extents as M

    fns = {}
    for name, params in _declarations(HEADER).items():
        bufs = [p for p in params if "*" in p and not HANDLE.search(p)]
        if bufs:
            fns[name] = bufs
    assert not (set(M.GATED_MATRIX) & set(EXEMPT)) and not (HOST_ONLY & set(EXEMPT)) and not (HOST_ONLY & set(M.GATED_MATRIX))
    for name in fns:
        assert name in M.GATED_MATRIX or name in HOST_ONLY or name in EXEMPT, f"{name}{fns[name]}: not covered and not exempt"
    for name in list(M.GATED_MATRIX) + list(EXEMPT) + list(HOST_ONLY):
        assert name in fns, f"{name}: listed, but the header has no such function with a caller's buffer"
    for name, test in M.GATED_MATRIX.items():
        assert all(callable(getattr(M, t, None)) for t in test.split()), (name, test)


def test_the_host_twin_stays_inside_its_extents():
    w = T.short_walk()
    p = gated.params_of()
    for B in (1, 70, 700):
        for with_resets in (False, True):
            def call(q):
                C.memmove(q["state"], q["state0"], 24)
                return lib().og_track_host(q["state"], q["params"], q["best"], q["resets"], B, w["W"], w["H"], q["boxes"])
            out = G.run_guarded("og_track_host", f"B={B} resets={with_resets}", call,
                                {"state0": np.zeros(24, np.uint8), "params": np.frombuffer(bytes(p), np.uint8), "best": w["best"][:B],
                                 "resets": w["resets"][:B] if with_resets else None}, {"state": 24, "boxes": 16 * B})
            if with_resets:
                assert np.array_equal(out["boxes"].view(np.int32).reshape(B, 4), w["boxes"][:B])
                st = out["state"]
                assert (st[:8].view(np.float32).tolist() + st[8:].view(np.int32).tolist()) == list(w["states"][B - 1])


def test_null_and_misaligned_pointers_are_refused_without_a_device():
    """Argument checks come before the first HIP call and before the handle is looked at, so they can be held here."""
    l = lib()
    raw = np.zeros(8192, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 8
    frames, area, boxes, best, mask = base, base + 1024, base + 2048, base + 3072, base + 4096
    args = (1, 8, 8, 1, 256, 256, 256, 0.25, 0.5, None)
    for off in (1, 2):
        assert l.og_gated_stream_u8(None, frames, *args, area + off, boxes, best, mask) == OG_EINVAL
        assert b"area must be aligned to 4" in l.og_last_error()
        assert l.og_gated_stream_u8(None, frames, *args, area, boxes + off, best, mask) == OG_EINVAL
        assert l.og_gated_stream_u8(None, frames, *args, area, boxes, best + off, mask) == OG_EINVAL
        assert b"best must be aligned to 4" in l.og_last_error()
        assert l.og_track_boxes_dev(None, best + off, None, 1, 8, 8, boxes) == OG_EINVAL
        assert l.og_track_boxes_dev(None, best, None, 1, 8, 8, boxes + off) == OG_EINVAL
    ptrs = (C.c_void_p * 2)(frames, 0)
    assert l.og_gated_stream_frames_u8(None, C.addressof(ptrs) + 4, *args, area, boxes, best, mask) == OG_EINVAL
    assert b"frame_ptrs must be aligned to 8" in l.og_last_error()
    assert l.og_gated_stream_frames_u8(None, None, *args, area, boxes, best, mask) == OG_EINVAL
    assert l.og_gated_stream_u8(None, frames, 1, 8, 8, 2, 256, 256, 256, 0.25, 0.5, None, area, boxes, best, mask) == OG_EINVAL     # channels
    assert l.og_gated_stream_u8(None, frames, -1, 8, 8, 1, 256, 256, 256, 0.25, 0.5, None, area, boxes, best, mask) == OG_EINVAL
    assert l.og_gated_stream_u8(None, frames, *args, area, boxes, best, mask) == OG_EINVAL and b"null handle" in l.og_last_error()
    for fn in (l.og_gated_sync, l.og_gated_reset):
        assert fn(None) == OG_EINVAL
    assert l.og_gated_set_option(None, b"stage_kib", 1) == OG_EINVAL
    assert l.og_gated_set_params(None, best) == OG_EINVAL and l.og_gated_get_state(None, best) == OG_EINVAL
    assert l.og_gated_set_state(None, best) == OG_EINVAL
    assert not l.og_gated_create(None, None) and b"null handle" in l.og_last_error()
    l.og_gated_destroy(None)                                                     # a no-op
    # borrowed handles that are not finalized: OG_ESTATE's message, no handle
    u = l.og_unet_create((C.c_int * 4)(4, 8, 16, 32), 4, 1, 1)
    y = l.og_yolo_create(1)
    try:
        assert u and y
        assert not l.og_gated_create(u, y) and b"finalized" in l.og_last_error()
    finally:
        l.og_unet_destroy(u)
        l.og_yolo_destroy(y)
    assert not raw.any()


def test_the_dry_run_gives_micro_batches_and_bytes_that_do_not_grow_with_the_video():
    fb = 480 * 640 * 3
    kib = 16 * fb // 1024                                     # room for 16 frames
    a, bytes_a = gated.plan(64, 480, 640, 3, kib)
    b, bytes_b = gated.plan(6400, 480, 640, 3, kib)
    assert bytes_a == bytes_b == 2 * 16 * (480 * 640 * 4 + 41) + 24
    assert a == [(0, 16), (16, 16), (32, 16), (48, 16)] and len(b) == 400 and b[-1] == (6384, 16)
    mbs, _ = gated.plan(70, 96, 160, 3, 25 * 96 * 160 * 3 // 1024)                # 70 frames, 25 fit: three micro-batches, the last partial
    assert mbs == [(0, 25), (25, 25), (50, 20)]
    mbs, one = gated.plan(5, 1080, 1920, 3, 100)              # stage_kib below one frame: each frame is staged alone
    assert mbs == [(i, 1) for i in range(5)] and one == 2 * (1080 * 1920 * 4 + 41) + 24
    mbs, _ = gated.plan(10000, 8, 8, 1, 65536)                # small frames: at most 4096 per micro-batch
    assert mbs == [(0, 4096), (4096, 4096), (8192, 1808)]
    assert gated.plan(3, 256, 256, 3) == ([(0, 3)], 2 * 341 * (256 * 256 * 4 + 41) + 24)      # the default setting: room for 341 frames


def test_the_dry_run_refuses_bad_arguments():
    l = lib()
    out = C.create_string_buffer(64)
    n = C.c_longlong()
    assert l.og_gated_plan(0, 8, 8, 1, 64, out, 64, C.byref(n)) == OG_EINVAL
    assert l.og_gated_plan(1, 8, 8, 2, 64, out, 64, C.byref(n)) == OG_EINVAL
    assert l.og_gated_plan(1, 8, 8, 1, 0, out, 64, C.byref(n)) == OG_EINVAL
    assert l.og_gated_plan(1, 8, 8, 1, 64, None, 64, C.byref(n)) == OG_EINVAL
    assert l.og_gated_plan(1000, 8, 8, 1, 1, out, 64, C.byref(n)) == OG_EINVAL and b"does not fit" in l.og_last_error()
    assert l.og_gated_plan(1, 8, 8, 1, 64, out, 64, None) == 1 and out.value == b"0|1\n"


def test_the_new_sources_hold_no_inline_assembly():
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_gated.inc")).read()
    assert "asm" not in src
    kern = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_kernels.hpp")).read()
    new = kern[kern.index("The temporal tracker of the gated pipeline"):]
    assert "asm" not in new and "k_track_boxes" in new
