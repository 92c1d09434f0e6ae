"""The rules tests/test_gated_abi.py holds the fourth header to, on the eighth, include/openglottal_hip_gate.h: every function it
declares is exported and bound (`_lib.GATE_PROTOTYPES`) and vice versa; the seven older headers and their tables are untouched;
every function with a caller's buffer is in the extents matrix of tests/test_gpu_gate_extents.py, host only (and then held to its
extents in tests/test_gate_host.py) or exempt for a stated reason; misaligned and null pointers are refused before anything is
written; the dry run.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

from openglottal_amd import _lib, gated
from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL = -1
HEADER = "openglottal_hip_gate.h"

EXEMPT = {
    "og_gate_plan": "plan recorder: host text bounded by cap (test_the_dry_run_* below)",
}
HOST_ONLY = {"og_gate_select_host"}
HANDLE = re.compile(r"(og_gated|og_unet|og_yolo)\s*\*\s*\w+$")
OLDER = {"openglottal_hip.h": ("PROTOTYPES", 66), "openglottal_hip_crops.h": ("CROP_PROTOTYPES", 7), "openglottal_hip_classic.h": ("CLASSIC_PROTOTYPES", 20),
         "openglottal_hip_gated.h": ("GATED_PROTOTYPES", 13), "openglottal_hip_classic_tiled.h": ("TILED_PROTOTYPES", 4),
         "openglottal_hip_overlay.h": ("OVERLAY_PROTOTYPES", 11), "openglottal_hip_sweep.h": ("SWEEP_PROTOTYPES", 11)}


def _declarations(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_function_of_the_gate_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == {"og_gate_select_host", "og_gate_select_dev", "og_gate_gather_dev", "og_gate_scatter_dev", "og_gated_segment_kept_dev",
                         "og_gated_stream_kept_u8", "og_gated_stream_kept_frames_u8", "og_gate_plan"}
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        args = _lib.GATE_PROTOTYPES[name][1]
        assert list(getattr(l, name).argtypes or []) == args, name
        assert len(args) == len(decl[name]), name
    assert set(decl) == set(_lib.GATE_PROTOTYPES)
    older = set()
    for table, _ in OLDER.values():
        older |= set(getattr(_lib, table))
    assert not (set(_lib.GATE_PROTOTYPES) & older)
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "openglottal_hip.h"' in text and '#include "openglottal_hip_gated.h"' in text      # og_gated is the fourth header's
    assert "THE HOST WAITS FOR THIS EVENT AND FOR NOTHING ELSE" in text
    # the kept stream entries take the arguments of og_gated_stream_u8 plus the count
    plain = _declarations("openglottal_hip_gated.h")
    for kept, base in (("og_gated_stream_kept_u8", "og_gated_stream_u8"), ("og_gated_stream_kept_frames_u8", "og_gated_stream_frames_u8")):
        assert decl[kept][:-1] == plain[base] and decl[kept][-1] == "int32_t* n_kept_or_null"


def test_the_seven_older_headers_still_equal_their_tables_and_are_unchanged():
    for header, (table, count) in OLDER.items():
        assert set(_declarations(header)) == set(getattr(_lib, table)), header
        assert len(getattr(_lib, table)) == count, header
        text = open(os.path.join(ROOT, "include", header)).read()
        assert "og_gate_" not in text and "_kept" not in text, header


def test_every_gate_entry_with_a_caller_buffer_is_in_the_matrix_host_only_or_exempt():
    import test_gpu_gate_extents as M

    fns = {}
    for name, params in _declarations(HEADER).items():
        bufs = [p for p in params if "*" in p and not HANDLE.search(p)]
        if bufs:
            fns[name] = bufs
    assert not (set(M.GATE_MATRIX) & set(EXEMPT)) and not (HOST_ONLY & set(EXEMPT)) and not (HOST_ONLY & set(M.GATE_MATRIX))
    for name in fns:
        assert name in M.GATE_MATRIX or name in HOST_ONLY or name in EXEMPT, f"{name}{fns[name]}: not covered and not exempt"
    for name in list(M.GATE_MATRIX) + list(EXEMPT) + list(HOST_ONLY):
        assert name in fns, f"{name}: listed, but the header has no such function with a caller's buffer"
    for name, test in M.GATE_MATRIX.items():
        assert all(callable(getattr(M, t, None)) for t in test.split()), (name, test)


def test_null_and_misaligned_pointers_are_refused_without_a_device():
    """Argument checks come before the first HIP call and before the handle is looked at, so they can be held here."""
    l = lib()
    raw = np.zeros(8192, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 8
    frames, area, boxes, best, mask, keep, count = base, base + 1024, base + 2048, base + 3072, base + 4096, base + 5120, base + 6144
    args = (1, 8, 8, 1, 256, 256, 256, 0.25, 0.5, None)
    for off in (1, 2):
        for fn in (l.og_gated_stream_kept_u8, l.og_gated_stream_kept_frames_u8):
            assert fn(None, frames, *args, area + off, boxes, best, mask, count) == OG_EINVAL
            assert b"area must be aligned to 4" in l.og_last_error()
            assert fn(None, frames, *args, area, boxes + off, best, mask, count) == OG_EINVAL
            assert fn(None, frames, *args, area, boxes, best + off, mask, count) == OG_EINVAL
            assert fn(None, frames, *args, area, boxes, best, mask, count + off) == OG_EINVAL
            assert b"n_kept must be aligned to 4" in l.og_last_error()
        assert l.og_gate_select_dev(None, boxes + off, 1, keep, count) == OG_EINVAL and b"boxes_dev must be aligned to 4" in l.og_last_error()
        assert l.og_gate_select_dev(None, boxes, 1, keep + off, count) == OG_EINVAL
        assert l.og_gate_select_dev(None, boxes, 1, keep, count + off) == OG_EINVAL
        assert l.og_gate_gather_dev(None, frames, 16, keep + off, 1, mask) == OG_EINVAL and b"keep_dev must be aligned to 4" in l.og_last_error()
        assert l.og_gate_scatter_dev(None, frames, 16, keep + off, 1, 1, mask) == OG_EINVAL
        assert l.og_gated_segment_kept_dev(None, frames, 1, 8, 8, 1, 256, 256, 0.5, boxes + off, mask, area, count) == OG_EINVAL
        assert l.og_gated_segment_kept_dev(None, frames, 1, 8, 8, 1, 256, 256, 0.5, boxes, mask, area + off, count) == OG_EINVAL
        assert l.og_gated_segment_kept_dev(None, frames, 1, 8, 8, 1, 256, 256, 0.5, boxes, mask, area, count + off) == OG_EINVAL
        assert l.og_gate_select_host(boxes + off, 1, keep) == OG_EINVAL and l.og_gate_select_host(boxes, 1, keep + off) == OG_EINVAL
    ptrs = (C.c_void_p * 2)(frames, 0)
    assert l.og_gated_stream_kept_frames_u8(None, C.addressof(ptrs) + 4, *args, area, boxes, best, mask, count) == OG_EINVAL
    assert b"frame_ptrs must be aligned to 8" in l.og_last_error()
    assert l.og_gated_stream_kept_frames_u8(None, None, *args, area, boxes, best, mask, count) == OG_EINVAL
    assert l.og_gated_stream_kept_u8(None, frames, 1, 8, 8, 2, 256, 256, 256, 0.25, 0.5, None, area, boxes, best, mask, count) == OG_EINVAL     # channels
    assert l.og_gated_stream_kept_u8(None, frames, -1, 8, 8, 1, 256, 256, 256, 0.25, 0.5, None, area, boxes, best, mask, count) == OG_EINVAL
    assert l.og_gated_stream_kept_u8(None, frames, *args, area, boxes, best, mask, count) == OG_EINVAL and b"null handle" in l.og_last_error()
    # null buffers, bad sizes, then the null handle -- in that order
    assert l.og_gate_select_dev(None, None, 1, keep, count) == OG_EINVAL and b"null buffer" in l.og_last_error()
    assert l.og_gate_select_dev(None, boxes, 1, keep, None) == OG_EINVAL and b"null buffer" in l.og_last_error()
    assert l.og_gate_select_dev(None, boxes, -1, keep, count) == OG_EINVAL and l.og_gate_select_dev(None, boxes, (1 << 20) + 1, keep, count) == OG_EINVAL
    assert l.og_gate_select_dev(None, boxes, 1, keep, count) == OG_EINVAL and b"null handle" in l.og_last_error()
    assert l.og_gate_gather_dev(None, None, 16, keep, 1, mask) == OG_EINVAL and b"null buffer" in l.og_last_error()
    assert l.og_gate_gather_dev(None, frames, 0, keep, 1, mask) == OG_EINVAL and b"row_bytes" in l.og_last_error()
    assert l.og_gate_gather_dev(None, frames, 8192 * 8192 * 3 + 1, keep, 1, mask) == OG_EINVAL and b"row_bytes" in l.og_last_error()
    assert l.og_gate_gather_dev(None, frames, 16, keep, -1, mask) == OG_EINVAL
    assert l.og_gate_gather_dev(None, frames, 16, keep, 1, mask) == OG_EINVAL and b"null handle" in l.og_last_error()
    assert l.og_gate_scatter_dev(None, frames, 16, keep, 2, 1, mask) == OG_EINVAL and b"n must be" in l.og_last_error()
    assert l.og_gate_scatter_dev(None, frames, 16, keep, 1, 1, None) == OG_EINVAL and b"null buffer" in l.og_last_error()
    assert l.og_gate_scatter_dev(None, frames, 16, keep, 1, 1, mask) == OG_EINVAL and b"null handle" in l.og_last_error()
    assert l.og_gated_segment_kept_dev(None, frames, 1, 8, 8, 2, 256, 256, 0.5, boxes, mask, area, count) == OG_EINVAL
    assert l.og_gated_segment_kept_dev(None, frames, 1, 8, 8, 1, 256, 256, 0.5, boxes, mask, area, count) == OG_EINVAL
    assert b"null handle" in l.og_last_error()
    assert l.og_gate_select_host(None, 1, keep) == OG_EINVAL and l.og_gate_select_host(boxes, 1, None) == OG_EINVAL
    assert l.og_gate_select_host(boxes, -1, keep) == OG_EINVAL and l.og_gate_select_host(None, 0, None) == 0
    assert not raw.any()


def test_the_dry_run_gives_og_gated_plans_micro_batches_and_the_bytes_of_the_formula():
    fb = 480 * 640 * 3
    kib = 16 * fb // 1024                                     # room for 16 frames
    for B in (64, 6400):
        for with_mask in (False, True):
            mbs, nbytes = gated.gate_plan(B, 480, 640, 3, kib, with_mask)
            plain, plain_bytes = gated.plan(B, 480, 640, 3, kib)
            assert mbs == plain and plain_bytes == 2 * 16 * (480 * 640 * 4 + 41) + 24          # og_gated_plan's own output is unchanged
            px = 480 * 640 * (3 + (1 if with_mask else 0))
            assert nbytes == 2 * 16 * (px + 41) + 24 + 2 * (16 * px + 16 * 24 + 4), (B, with_mask)     # ... and does not grow with B
    assert gated.gate_plan(70, 96, 160, 3, 25 * 96 * 160 * 3 // 1024)[0] == [(0, 25), (25, 25), (50, 20)]
    mbs, one = gated.gate_plan(5, 1080, 1920, 3, 100)          # stage_kib below one frame: each frame is staged alone
    assert mbs == [(i, 1) for i in range(5)] and one == 2 * (1080 * 1920 * 3 + 41) + 24 + 2 * (1080 * 1920 * 3 + 24 + 4)
    assert gated.gate_plan(10000, 8, 8, 1, 65536)[0] == [(0, 4096), (4096, 4096), (8192, 1808)]


def test_the_dry_run_refuses_bad_arguments():
    l = lib()
    out = C.create_string_buffer(64)
    n = C.c_longlong()
    assert l.og_gate_plan(0, 8, 8, 1, 64, 0, out, 64, C.byref(n)) == OG_EINVAL
    assert l.og_gate_plan(1, 8, 8, 2, 64, 0, out, 64, C.byref(n)) == OG_EINVAL
    assert l.og_gate_plan(1, 8, 8, 1, 0, 0, out, 64, C.byref(n)) == OG_EINVAL
    assert l.og_gate_plan(1, 8, 8, 1, 64, 2, out, 64, C.byref(n)) == OG_EINVAL and b"with_mask" in l.og_last_error()
    assert l.og_gate_plan(1, 8, 8, 1, 64, 0, None, 64, C.byref(n)) == OG_EINVAL
    assert l.og_gate_plan(1000, 8, 8, 1, 1, 0, out, 64, C.byref(n)) == OG_EINVAL and b"does not fit" in l.og_last_error()
    assert l.og_gate_plan(1, 8, 8, 1, 64, 1, out, 64, None) == 1 and out.value == b"0|1\n"


def test_the_gate_sources_are_plain_cpp_and_share_one_rule():
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_gate.inc")).read()
    assert "asm" not in src and "atomic" not in src
    for k in ("k_gate_select", "k_gate_gather", "k_gate_scatter"):
        assert f"void {k}(" in src, k
    api = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_api.hip")).read()
    assert api.index('#include "og_gated.inc"') < api.index('#include "og_gate.inc"')
    kern = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_kernels.hpp")).read()
    assert "inline bool og_gate_keeps(" in kern and src.count("og_gate_keeps(") == 2          # the kernel and the host twin call it
