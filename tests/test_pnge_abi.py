"""The rules tests/test_png_abi.py holds the twelfth header to, on the thirteenth, include_enc/openglottal_hip_pnge.h: every function
it declares is exported and bound (`_lib.PNGE_PROTOTYPES`) and vice versa, the table is disjoint from the twelve older ones and those
keep their sizes, every argument and alignment check comes before the first HIP call, and B = 0 is a no-op.  The listing of
include_enc/ is NOT pinned: the next header may join this one.  No GPU."""
import ctypes as C
import os

import numpy as np

from openglottal_amd import _lib
from openglottal_amd import png as P
from openglottal_amd._lib import lib
from test_mjpd_abi import OLDER, ROOT, _declarations

OG_EINVAL = -1
HEADER = os.path.join(ROOT, "include_enc", "openglottal_hip_pnge.h")
NAMES = {"og_pnge_limit", "og_pnge_bound", "og_pnge_filter_host", "og_pnge_deflate_host", "og_pnge_encode_host", "og_pnge_create",
         "og_pnge_destroy", "og_pnge_sync", "og_pnge_set_chunk", "og_pnge_set_segment", "og_pnge_encode_u8_dev", "og_pnge_encode_stream_u8",
         "og_pnge_label_bbox_host", "og_pnge_label_bbox_u8_dev", "og_pnge_crop_tiles_u8_dev", "og_pnge_plan"}


def test_every_function_of_the_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == NAMES == set(_lib.PNGE_PROTOTYPES)
    assert all(n.startswith("og_pnge_") for n in decl)
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        args = _lib.PNGE_PROTOTYPES[name][1]
        assert list(getattr(l, name).argtypes or []) == args, name
        assert len(args) == (0 if decl[name] == ["void"] else len(decl[name])), name
    text = open(HEADER).read()
    assert '#include "../include_ext/openglottal_hip_png.h"' in text and "UNPINNED" in text and "OUT OF SCOPE" in text and "BOUND" in text
    for word in ("palette", "alpha", "16-bit", "Adam7", "mixed shapes"):
        assert word in text, word


def test_the_twelve_older_tables_keep_their_sizes():
    seen = set(_lib.PNGE_PROTOTYPES)
    older = dict(OLDER, **{"decode/openglottal_hip_mjpd.h": ("MJPD_PROTOTYPES", 13), "split/openglottal_hip_mjps.h": ("MJPS_PROTOTYPES", 4)})
    for header, (table, count) in older.items():
        t = getattr(_lib, table)
        assert len(t) == count and set(_declarations(os.path.join(ROOT, "include", header))) == set(t), header
        assert not (set(t) & seen), header
        seen |= set(t)
    assert len(_lib.PNG_PROTOTYPES) == 13 and not (set(_lib.PNG_PROTOTYPES) & seen)
    assert set(_declarations(os.path.join(ROOT, "include_ext", "openglottal_hip_png.h"))) == set(_lib.PNG_PROTOTYPES)
    api = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_api.hip")).read()
    assert api.count('#include "og_pnge.inc"') == 1 and api.index('#include "og_png.inc"') < api.index('#include "og_pnge.inc"')
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_pnge.inc")).read()
    assert "asm" not in src and all(k in src for k in ("k_pnge_filter", "k_pnge_segment", "k_pnge_offsets", "k_pnge_place", "k_label_bbox",
                                                       "og_png_adler_part", "og_png_adler_join", "OG_PNG_HOST_ONLY", "og_two_slot"))
    assert "include_enc" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_limits_and_bound():
    l = lib()
    assert [l.og_pnge_limit(i) for i in range(7)] == [l.og_png_limit(0), 1024, 64, 32768, 32768, 128, 57]
    assert 0 < 2 * l.og_pnge_limit(7) <= 160 << 10                             # two workgroups of k_pnge_segment fit a CU's LDS
    assert l.og_pnge_limit(8) == -1 and l.og_pnge_limit(-1) == -1
    for H, W, Cn, S in ((1, 1, 1, 64), (256, 256, 1, 32768), (256, 256, 3, 32768), (5, 40, 3, 64), (480, 640, 1, 256)):
        N = H * (1 + W * Cn)
        assert l.og_pnge_bound(H, W, Cn, S) == 57 + 2 + 4 + N + 5 * (-(-N // S))
    for bad in ((0, 4, 1, 64), (4, 0, 1, 64), (4, 4, 2, 64), (4, 4, 4, 64), (4, 4, 1, 32), (4, 4, 1, 96), (4, 4, 1, 65536), (4097, 4096, 1, 64)):
        assert l.og_pnge_bound(*bad) == -1 and l.og_last_error()
    e = P.PngEncoder()
    assert (e.chunk, e.segment) == (128, 32768)


def test_the_handle_refuses_bad_arguments_without_a_device():
    """Argument checks come before the first HIP call, so they can be held here."""
    l = lib()
    h = l.og_pnge_create()
    assert h
    try:
        raw = np.zeros(1 << 16, np.uint8)
        base = raw.ctypes.data + (-raw.ctypes.data) % 8
        frames, out, sizes, total, boxes = (base + 8192 * i for i in range(5))
        raw[:64] = np.arange(64)
        before = raw.copy()
        B, H, W, Cn = 2, 4, 8, 1
        cap = B * l.og_pnge_bound(H, W, Cn, 32768)
        for fn in (l.og_pnge_encode_u8_dev, l.og_pnge_encode_stream_u8):
            assert fn(None, frames, B, H, W, Cn, out, cap, sizes, total) == OG_EINVAL and b"null handle" in l.og_last_error()
            assert fn(h, frames, B, H, W, Cn, out, cap - 1, sizes, total) == OG_EINVAL and b"cap is below" in l.og_last_error()
            assert str(cap).encode() in l.og_last_error()
            assert fn(h, frames, -1, H, W, Cn, out, cap, sizes, total) == OG_EINVAL
            for ch in (0, 2, 4):
                assert fn(h, frames, B, H, W, ch, out, cap, sizes, total) == OG_EINVAL and b"C must be" in l.og_last_error()
            assert fn(h, frames, B, 0, W, Cn, out, cap, sizes, total) == OG_EINVAL and fn(h, frames, B, H, 0, Cn, out, cap, sizes, total) == OG_EINVAL
            assert fn(h, frames, 1, 4097, 4096, Cn, out, 1 << 40, sizes, total) == OG_EINVAL
            for off in (1, 2, 3):
                assert fn(h, frames, B, H, W, Cn, out, cap, sizes + off, total) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
            for off in (1, 2, 4, 7):
                assert fn(h, frames, B, H, W, Cn, out, cap, sizes, total + off) == OG_EINVAL and b"aligned to 8" in l.og_last_error()
            for i in (0, 5, 7, 8):
                args = [frames, B, H, W, Cn, out, cap, sizes, total]
                args[i] = None
                assert fn(h, *args) == OG_EINVAL, i
            assert fn(h, frames, 0, H, W, Cn, out, 0, sizes, total) == 0     # B = 0: nothing to do
        view = np.frombuffer(raw, np.int64, 1, total - raw.ctypes.data)
        view[0] = 9
        assert l.og_pnge_encode_stream_u8(h, frames, 0, H, W, Cn, out, 0, sizes, total) == 0 and view[0] == 0      # no frames: no bytes
        assert np.array_equal(raw, before)                                    # nothing touched a device or a buffer
        bb, ct = l.og_pnge_label_bbox_u8_dev, l.og_pnge_crop_tiles_u8_dev
        assert bb(None, frames, 1, H, W, boxes) == OG_EINVAL and bb(h, None, 1, H, W, boxes) == OG_EINVAL and bb(h, frames, 1, H, W, None) == OG_EINVAL
        assert bb(h, frames, 1, 0, W, boxes) == OG_EINVAL and bb(h, frames, -1, H, W, boxes) == OG_EINVAL and bb(h, frames, 0, H, W, boxes) == 0
        assert bb(h, frames, 1, H, W, boxes + 2) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
        assert ct(None, frames, 1, H, W, 1, boxes, 32, out) == OG_EINVAL and ct(h, frames, 1, H, W, 2, boxes, 32, out) == OG_EINVAL
        assert ct(h, frames, 1, H, W, 1, boxes, 0, out) == OG_EINVAL and ct(h, frames, 1, H, W, 1, boxes + 1, 32, out) == OG_EINVAL
        assert ct(h, None, 1, H, W, 1, boxes, 32, out) == OG_EINVAL and ct(h, frames, 1, H, W, 1, None, 32, out) == OG_EINVAL
        assert ct(h, frames, 1, H, W, 1, boxes, 32, None) == OG_EINVAL and ct(h, frames, 0, H, W, 1, boxes, 32, out) == 0
        assert np.array_equal(raw, before)
        assert l.og_pnge_set_chunk(h, 0) == OG_EINVAL and l.og_pnge_set_chunk(h, 1025) == OG_EINVAL and l.og_pnge_set_chunk(h, 7) == 0
        for S in (0, 32, 96, 65536, -64):
            assert l.og_pnge_set_segment(h, S) == OG_EINVAL and b"power of two" in l.og_last_error()
        assert l.og_pnge_set_segment(h, 64) == 0 and l.og_pnge_set_segment(None, 64) == OG_EINVAL
        small = B * l.og_pnge_bound(4, 31, 1, 32768)                          # the cap rule follows the handle's segment: two of them now
        assert small < B * l.og_pnge_bound(4, 31, 1, 64)
        assert l.og_pnge_encode_stream_u8(h, frames, B, 4, 31, 1, out, small, sizes, total) == OG_EINVAL and b"cap is below" in l.og_last_error()
        assert l.og_pnge_set_chunk(None, 4) == OG_EINVAL and l.og_pnge_sync(None) == OG_EINVAL
        assert l.og_pnge_sync(h) == 0                                         # no stream yet: nothing to wait for
    finally:
        l.og_pnge_destroy(h)
    l.og_pnge_destroy(None)


def test_the_host_entries_refuse_bad_arguments_and_write_nothing():
    l = lib()
    f = np.arange(32, dtype=np.uint8)
    out, n = np.zeros(512, np.uint8), np.zeros(2, np.uint64)
    size = np.zeros(2, np.int32)
    enc, filt, defl = l.og_pnge_encode_host, l.og_pnge_filter_host, l.og_pnge_deflate_host
    bound = l.og_pnge_bound(4, 8, 1, 64)
    assert enc(f.ctypes.data, 4, 8, 1, 64, out.ctypes.data, bound - 1, size.ctypes.data) == OG_EINVAL and b"cap is below" in l.og_last_error()
    assert enc(f.ctypes.data, 4, 8, 2, 64, out.ctypes.data, bound, size.ctypes.data) == OG_EINVAL
    assert enc(f.ctypes.data, 4, 8, 1, 48, out.ctypes.data, bound, size.ctypes.data) == OG_EINVAL
    assert enc(None, 4, 8, 1, 64, out.ctypes.data, bound, size.ctypes.data) == OG_EINVAL and enc(f.ctypes.data, 4, 8, 1, 64, None, bound, size.ctypes.data) == OG_EINVAL
    assert enc(f.ctypes.data, 4, 8, 1, 64, out.ctypes.data, bound, None) == OG_EINVAL
    assert enc(f.ctypes.data, 4, 8, 1, 64, out.ctypes.data, bound, size.ctypes.data + 2) == OG_EINVAL
    assert filt(f.ctypes.data, 4, 8, 1, out.ctypes.data, 35) == OG_EINVAL and filt(None, 4, 8, 1, out.ctypes.data, 36) == OG_EINVAL
    assert filt(f.ctypes.data, 4, 8, 1, None, 36) == OG_EINVAL and filt(f.ctypes.data, 4, 8, 5, out.ctypes.data, 360) == OG_EINVAL
    assert defl(f.ctypes.data, 32, 64, out.ctypes.data, 6 + 32 + 5 - 1, n.ctypes.data) == OG_EINVAL
    assert defl(f.ctypes.data, 0, 64, out.ctypes.data, 64, n.ctypes.data) == OG_EINVAL and defl(f.ctypes.data, 32, 63, out.ctypes.data, 64, n.ctypes.data) == OG_EINVAL
    assert defl(None, 32, 64, out.ctypes.data, 64, n.ctypes.data) == OG_EINVAL and defl(f.ctypes.data, 32, 64, out.ctypes.data, 64, n.ctypes.data + 4) == OG_EINVAL
    box = np.zeros(6, np.int32)
    bb = l.og_pnge_label_bbox_host
    assert bb(None, 4, 8, box.ctypes.data) == OG_EINVAL and bb(f.ctypes.data, 4, 8, None) == OG_EINVAL and bb(f.ctypes.data, 0, 8, box.ctypes.data) == OG_EINVAL
    assert bb(f.ctypes.data, 4, 8, box.ctypes.data + 1) == OG_EINVAL
    assert not out.any() and not size.any() and not n.any() and not box.any()
    assert enc(f.ctypes.data, 4, 8, 1, 64, out.ctypes.data, bound, size.ctypes.data) == 0 and 57 < size[0] <= bound and not out[size[0]:].any()
    assert bb(f.ctypes.data, 4, 8, box.ctypes.data) == 0 and box.tolist() == [0, 0, 8, 4, 0, 0]


def test_label_boxes_on_the_host():
    def box(lab):
        b = np.zeros(4, np.int32)
        assert lib().og_pnge_label_bbox_host(lab.ctypes.data, lab.shape[0], lab.shape[1], b.ctypes.data) == 0
        return b.tolist()

    lab = np.zeros((9, 13), np.uint8)
    assert box(lab) == [0, 0, 0, 0]
    lab[4, 6] = 1
    assert box(lab) == [6, 4, 7, 5]                                          # one pixel: label > 0, not only 255
    lab[0, 12] = lab[8, 0] = 255
    assert box(lab) == [0, 0, 13, 9]
    lab[:] = 0
    lab[2:5, 3:9] = 200
    assert box(lab) == [3, 2, 9, 5]
