"""The rules tests/test_classic_abi.py holds the third header to, on the sixth, include/openglottal_hip_overlay.h: every function it
declares is exported and bound (`_lib.OVERLAY_PROTOTYPES`) and vice versa, the table is disjoint from the five older ones, every
argument check comes before the first HIP call, and the host entries stay inside guard-zoned buffers.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import buffer_guard as G
import overlay_cases as OC
from openglottal_amd import _lib
from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL = -1
HEADER = "openglottal_hip_overlay.h"
STYLE = {"none": 0, "contour": 1, "fill": 2}


def _declarations(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_function_of_the_overlay_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == {"og_overlay_limit", "og_outline_host", "og_overlay_host", "og_overlay_create", "og_overlay_destroy",
                         "og_overlay_sync", "og_overlay_set_chunk", "og_overlay_u8_dev", "og_overlay_stream_u8",
                         "og_overlay_stream_frames_u8", "og_overlay_plan"}
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        args = _lib.OVERLAY_PROTOTYPES[name][1]
        assert list(getattr(l, name).argtypes or []) == args, name
        assert len(args) == (0 if decl[name] == ["void"] else len(decl[name])), name
    assert set(decl) == set(_lib.OVERLAY_PROTOTYPES)
    older = (set(_lib.PROTOTYPES) | set(_lib.CROP_PROTOTYPES) | set(_lib.CLASSIC_PROTOTYPES) | set(_lib.GATED_PROTOTYPES)
             | set(_lib.TILED_PROTOTYPES))
    assert not (set(_lib.OVERLAY_PROTOTYPES) & older)
    assert '#include "openglottal_hip.h"' in open(os.path.join(ROOT, "include", HEADER)).read()


def test_limits():
    l = lib()
    assert l.og_overlay_limit(0) == l.og_classic_tiled_limit(0)           # nothing larger has been labelled by these kernels
    assert l.og_overlay_limit(1) == 3 and l.og_overlay_limit(2) == 1024
    assert l.og_overlay_limit(3) == -1 and l.og_overlay_limit(-1) == -1


def test_the_handle_refuses_bad_arguments_without_a_device():
    """Argument checks come before the first HIP call, so they can be held here."""
    l = lib()
    h = l.og_overlay_create()
    assert h
    try:
        raw = np.zeros(8192, np.uint8)
        base = raw.ctypes.data + (-raw.ctypes.data) % 8
        frames, masks, boxes, out = base, base + 1024, base + 2048, base + 4096
        limit = l.og_overlay_limit(0)
        ptrs = (C.c_void_p * 2)(frames, 0)
        for fn in (l.og_overlay_u8_dev, l.og_overlay_stream_u8, l.og_overlay_stream_frames_u8):
            f = C.addressof(ptrs) if fn is l.og_overlay_stream_frames_u8 else frames
            assert fn(None, f, 1, 8, 8, 1, masks, boxes, 2, out) == OG_EINVAL
            assert b"null handle" in l.og_last_error()
            for style in (-1, 3, 7):
                assert fn(h, f, 1, 8, 8, 1, masks, boxes, style, out) == OG_EINVAL
                assert b"style" in l.og_last_error()
            for ch in (0, 2, 4):
                assert fn(h, f, 1, 8, 8, ch, masks, boxes, 2, out) == OG_EINVAL
                assert b"channels" in l.og_last_error()
            assert fn(h, f, 1, 1, limit + 1, 1, masks, boxes, 2, out) == OG_EINVAL
            assert str(limit).encode() in l.og_last_error()
            for off in (1, 2, 3):
                assert fn(h, f, 1, 8, 8, 1, masks, boxes + off, 2, out) == OG_EINVAL
                assert b"must be aligned to 4" in l.og_last_error()
            assert fn(h, f, -1, 8, 8, 1, masks, boxes, 2, out) == OG_EINVAL
            assert fn(h, f, 1, 0, 8, 1, masks, boxes, 2, out) == OG_EINVAL
            assert fn(h, f, 0, 8, 8, 1, masks, boxes, 2, out) == 0                # B = 0: nothing to do
            assert fn(h, f, 1, 8, 8, 1, masks, boxes, 2, None) == OG_EINVAL       # out is required
        assert l.og_overlay_stream_frames_u8(h, C.addressof(ptrs) + 4, 1, 8, 8, 1, masks, boxes, 2, out) == OG_EINVAL
        assert l.og_overlay_stream_frames_u8(h, C.addressof(ptrs), 2, 8, 8, 1, masks, boxes, 2, out) == OG_EINVAL     # frame_ptrs[1] is null
        assert l.og_overlay_stream_frames_u8(h, None, 1, 8, 8, 1, masks, boxes, 2, out) == OG_EINVAL
        assert l.og_overlay_stream_u8(h, None, 1, 8, 8, 1, masks, boxes, 2, out) == OG_EINVAL
        assert l.og_overlay_set_chunk(h, 0) == OG_EINVAL and l.og_overlay_set_chunk(h, 1025) == OG_EINVAL and l.og_overlay_set_chunk(h, 7) == 0
        assert l.og_overlay_set_chunk(None, 4) == OG_EINVAL and l.og_overlay_sync(None) == OG_EINVAL
        assert l.og_overlay_sync(h) == 0                                      # no stream yet: nothing to wait for
        assert not raw.any()                                                  # nothing touched a device or a buffer
    finally:
        l.og_overlay_destroy(h)
    l.og_overlay_destroy(None)


def test_the_host_entries_refuse_bad_arguments_and_write_nothing():
    buf = G.Region("b", 1 << 16, "host", G.guard_bytes(1 << 16), G.GUARD_FILL)
    a = buf.ptr
    frame, mask, box, out = a, a + 4096, a + 8192, a + 16384
    before = buf.snapshot()
    l = lib()
    limit = l.og_overlay_limit(0)
    for off in (1, 2, 3):
        assert l.og_overlay_host(frame, 8, 8, 3, mask, box + off, 2, out) == OG_EINVAL
    assert l.og_overlay_host(frame, 8, 8, 2, mask, box, 2, out) == OG_EINVAL
    assert l.og_overlay_host(frame, 8, 8, 3, mask, box, 3, out) == OG_EINVAL
    assert l.og_overlay_host(frame, 0, 8, 3, mask, box, 2, out) == OG_EINVAL
    assert l.og_overlay_host(frame, 1, limit + 1, 1, mask, box, 2, out) == OG_EINVAL
    assert l.og_overlay_host(None, 8, 8, 3, mask, box, 2, out) == OG_EINVAL
    assert l.og_overlay_host(frame, 8, 8, 3, mask, box, 2, None) == OG_EINVAL
    assert l.og_outline_host(None, 8, 8, out) == OG_EINVAL and l.og_outline_host(mask, 8, 8, None) == OG_EINVAL
    assert l.og_outline_host(mask, 8, 0, out) == OG_EINVAL and l.og_outline_host(mask, 1, limit + 1, out) == OG_EINVAL
    assert np.array_equal(buf.snapshot(), before)
    assert l.og_overlay_host(frame + 1, 8, 8, 3, mask + 3, box, 2, out + 5) == 0      # u8 buffers: any address


def test_host_entries_stay_inside_their_extents():
    rs = np.random.RandomState(4)
    for H, W in ((1, 1), (7, 13), (40, 56)):
        m = ((rs.rand(H, W) < 0.6) * 255).astype(np.uint8)
        out = G.run_guarded("og_outline_host", f"{H}x{W}", lambda p: lib().og_outline_host(p["mask"], H, W, p["out"]), {"mask": m},
                            {"out": H * W})
        assert np.array_equal(out["out"].reshape(H, W) > 0, OC.outline(m))
        for ch in (1, 3):
            f = OC.frames_for(1, H, W, ch, seed=H)[0]
            for style in OC.STYLES:
                for name, box in OC.box_cases(H, W) + [("no-boxes", None)]:
                    for mask in (m, None):
                        out = G.run_guarded("og_overlay_host", f"{H}x{W} ch={ch} {style} {name} mask={mask is not None}",
                                            lambda p: lib().og_overlay_host(p["frame"], H, W, ch, p["mask"], p["box"], STYLE[style], p["out"]),
                                            {"frame": f, "mask": mask, "box": None if box is None else np.array(box, np.int32)},
                                            {"out": H * W * 3})
                        want = OC.overlay(f, mask, OC.ABSENT if box is None else box, style)
                        assert np.array_equal(out["out"].reshape(H, W, 3), want), (H, W, ch, style, name)


def test_the_overlay_sources_hold_no_inline_assembly():
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_overlay.inc")).read()
    assert "asm" not in src and "k_overlay" in src
    kern = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_kernels.hpp")).read()
    new = kern[kern.index("Annotated frames (scripts/infer.py"):]
    assert "asm" not in new and "k_overlay" in new
    twin = kern[kern.index("k_tblob_background for a caller's MASK"):kern.index("// og_uf_union over the pixel pairs that straddle this tile's")]
    assert "asm" not in twin and "k_tblob_background_mask" in twin
