"""The rules tests/test_overlay_abi.py holds the sixth header to, on the ninth, include/openglottal_hip_mjpeg.h: every function it
declares is exported and bound (`_lib.MJPEG_PROTOTYPES`) and vice versa, the table is disjoint from the eight older ones and those are
untouched, every argument check comes before the first HIP call, and the host entries stay inside guard-zoned buffers.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import buffer_guard as G
import mjpeg_cases as MC
from openglottal_amd import _lib
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import OpenGlottalHipError, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL = -1
HEADER = "openglottal_hip_mjpeg.h"
OLDER = {"openglottal_hip.h": ("PROTOTYPES", 66), "openglottal_hip_crops.h": ("CROP_PROTOTYPES", 7),
         "openglottal_hip_classic.h": ("CLASSIC_PROTOTYPES", 20), "openglottal_hip_gated.h": ("GATED_PROTOTYPES", 13),
         "openglottal_hip_classic_tiled.h": ("TILED_PROTOTYPES", 4), "openglottal_hip_overlay.h": ("OVERLAY_PROTOTYPES", 11),
         "openglottal_hip_sweep.h": ("SWEEP_PROTOTYPES", 11), "openglottal_hip_gate.h": ("GATE_PROTOTYPES", 8)}


def _declarations(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_function_of_the_mjpeg_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == {"og_mjpeg_limit", "og_jpeg_bound", "og_jpeg_tables_host", "og_jpeg_coefficients_host", "og_jpeg_encode_host",
                         "og_mjpeg_create", "og_mjpeg_destroy", "og_mjpeg_sync", "og_mjpeg_set_chunk", "og_mjpeg_set_quality",
                         "og_mjpeg_encode_u8_dev", "og_mjpeg_encode_stream_u8", "og_mjpeg_plan"}
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        args = _lib.MJPEG_PROTOTYPES[name][1]
        assert list(getattr(l, name).argtypes or []) == args, name
        assert len(args) == (0 if decl[name] == ["void"] else len(decl[name])), name
    assert set(decl) == set(_lib.MJPEG_PROTOTYPES)
    assert '#include "openglottal_hip.h"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert "UNPINNED" in open(os.path.join(ROOT, "include", HEADER)).read()           # parity with OpenCV's MJPG writer is not claimed


def test_the_eight_older_headers_and_tables_are_untouched():
    seen = set()
    for header, (table, count) in OLDER.items():
        t = getattr(_lib, table)
        assert len(t) == count and set(_declarations(header)) == set(t), header
        assert not (set(t) & set(_lib.MJPEG_PROTOTYPES)) and not (set(t) & seen), header
        seen |= set(t)
    assert len([f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")]) == 9
    api = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_api.hip")).read()
    assert api.count('#include "og_mjpeg.inc"') == 1 and api.index('#include "og_sweep.inc"') < api.index('#include "og_mjpeg.inc"')


def test_limits_and_the_bound():
    l = lib()
    assert [l.og_mjpeg_limit(i) for i in range(8)] == [1 << 24, 16, 1024, 1, 100, 19972, 629, 75]
    assert l.og_mjpeg_limit(8) == -1 and l.og_mjpeg_limit(-1) == -1
    ri, slot = l.og_mjpeg_limit(1), l.og_mjpeg_limit(5)
    block = 2 * ((63 * 26 + 22 + 7) // 8)                                 # a block after stuffing, worst case
    assert slot >= 3 * ri * block + 2 and slot % 4 == 0
    for H, W in ((1, 1), (8, 8), (13, 21), (256, 256), (1080, 1920)):
        M = ((H + 7) // 8) * ((W + 7) // 8)
        assert l.og_jpeg_bound(H, W) == 629 + M * 3 * block + 2 * ((M + ri - 1) // ri) + 2
    assert l.og_jpeg_bound(0, 8) == -1 and l.og_jpeg_bound(8, -1) == -1 and l.og_jpeg_bound(4097, 4096) == -1
    assert l.og_jpeg_bound(1, 65536) == -1 and b"16 bits" in l.og_last_error()
    assert l.og_jpeg_bound(4096, 4096) < 2 ** 31                          # sizes are int32


def test_the_handle_refuses_bad_arguments_without_a_device():
    """Argument checks come before the first HIP call, so they can be held here."""
    l = lib()
    h = l.og_mjpeg_create()
    assert h
    try:
        raw = np.zeros(1 << 16, np.uint8)
        base = raw.ctypes.data + (-raw.ctypes.data) % 8
        frames, sizes, total, out = base, base + 1024, base + 2048, base + 4096
        cap = l.og_jpeg_bound(8, 8)
        limit = l.og_mjpeg_limit(0)
        for fn in (l.og_mjpeg_encode_u8_dev, l.og_mjpeg_encode_stream_u8):
            assert fn(None, frames, 1, 8, 8, out, cap, sizes, total) == OG_EINVAL
            assert b"null handle" in l.og_last_error()
            assert fn(h, frames, 1, 8, 8, out, cap - 1, sizes, total) == OG_EINVAL
            assert b"cap is below" in l.og_last_error() and str(cap).encode() in l.og_last_error()
            assert fn(h, frames, 3, 8, 8, out, 3 * cap - 1, sizes, total) == OG_EINVAL      # B * bound
            assert fn(h, frames, 1, 8, 8, out, 0, sizes, total) == OG_EINVAL
            assert fn(h, frames, 1, 1, limit + 1, out, 1 << 40, sizes, total) == OG_EINVAL
            assert fn(h, frames, -1, 8, 8, out, cap, sizes, total) == OG_EINVAL
            assert fn(h, frames, 1, 0, 8, out, cap, sizes, total) == OG_EINVAL
            assert fn(h, frames, 1, 8, 0, out, cap, sizes, total) == OG_EINVAL
            for off in (1, 2, 3):
                assert fn(h, frames, 1, 8, 8, out, cap, sizes + off, total) == OG_EINVAL
                assert b"must be aligned to 4" in l.og_last_error()
            for off in (1, 2, 4, 7):
                assert fn(h, frames, 1, 8, 8, out, cap, sizes, total + off) == OG_EINVAL
                assert b"must be aligned to 8" in l.og_last_error()
            assert fn(h, None, 1, 8, 8, out, cap, sizes, total) == OG_EINVAL
            assert fn(h, frames, 1, 8, 8, None, cap, sizes, total) == OG_EINVAL
            assert fn(h, frames, 1, 8, 8, out, cap, None, total) == OG_EINVAL
            assert fn(h, frames, 1, 8, 8, out, cap, sizes, None) == OG_EINVAL
        assert l.og_mjpeg_encode_u8_dev(h, frames, 0, 8, 8, out, 0, sizes, total) == 0       # B = 0: nothing to do
        assert not raw.any()                                                  # nothing touched a device or a buffer
        view = np.frombuffer(raw, np.int64, 1, total - raw.ctypes.data)
        view[0] = 77
        assert l.og_mjpeg_encode_stream_u8(h, frames, 0, 8, 8, out, 0, sizes, total) == 0 and view[0] == 0      # no frames: no bytes
        for q in (0, 101, -5):
            assert l.og_mjpeg_set_quality(h, q) == OG_EINVAL and b"quality" in l.og_last_error()
        assert l.og_mjpeg_set_quality(h, 1) == 0 and l.og_mjpeg_set_quality(h, 100) == 0 and l.og_mjpeg_set_quality(None, 75) == OG_EINVAL
        assert l.og_mjpeg_set_chunk(h, 0) == OG_EINVAL and l.og_mjpeg_set_chunk(h, 1025) == OG_EINVAL and l.og_mjpeg_set_chunk(h, 7) == 0
        assert l.og_mjpeg_set_chunk(None, 4) == OG_EINVAL and l.og_mjpeg_sync(None) == OG_EINVAL
        assert l.og_mjpeg_sync(h) == 0                                        # no stream yet: nothing to wait for
    finally:
        l.og_mjpeg_destroy(h)
    l.og_mjpeg_destroy(None)


def test_the_python_layer_refuses_other_channel_counts_and_qualities():
    for shape in ((2, 8, 8), (2, 8, 8, 1), (2, 8, 8, 4)):
        with pytest.raises(OpenGlottalHipError, match="BGR"):
            MJ._bgr(np.zeros(shape, np.uint8), 4)
    with pytest.raises(OpenGlottalHipError, match="BGR"):
        MJ.encode_host(np.zeros((8, 8), np.uint8))
    for q in (0, 101):
        with pytest.raises(OpenGlottalHipError, match="quality"):
            MJ.Mjpeg(quality=q)
        with pytest.raises(OpenGlottalHipError, match="quality"):
            MJ.encode_host(np.zeros((8, 8, 3), np.uint8), q)
    e = MJ.Mjpeg()
    assert (e.quality, e.chunk) == (75, 128)


def test_the_host_entries_refuse_bad_arguments_and_write_nothing():
    buf = G.Region("b", 1 << 16, "host", G.guard_bytes(1 << 16), G.GUARD_FILL)
    a = buf.ptr
    frame, out, size, ql, qc, hdr = a, a + 4096, a + 32768, a + 33024, a + 33280, a + 36864
    before = buf.snapshot()
    l = lib()
    cap = l.og_jpeg_bound(8, 8)
    for q in (0, 101):
        assert l.og_jpeg_encode_host(frame, 8, 8, q, out, cap, size) == OG_EINVAL
        assert l.og_jpeg_coefficients_host(frame, 8, 8, q, out) == OG_EINVAL
        assert l.og_jpeg_tables_host(q, 8, 8, ql, qc, hdr, 1024, size) == OG_EINVAL
    assert l.og_jpeg_encode_host(frame, 8, 8, 75, out, cap - 1, size) == OG_EINVAL and b"cap is below" in l.og_last_error()
    assert l.og_jpeg_encode_host(None, 8, 8, 75, out, cap, size) == OG_EINVAL
    assert l.og_jpeg_encode_host(frame, 8, 8, 75, None, cap, size) == OG_EINVAL
    assert l.og_jpeg_encode_host(frame, 8, 8, 75, out, cap, None) == OG_EINVAL
    assert l.og_jpeg_encode_host(frame, 0, 8, 75, out, cap, size) == OG_EINVAL
    for off in (1, 2, 3):
        assert l.og_jpeg_encode_host(frame, 8, 8, 75, out, cap, size + off) == OG_EINVAL
        assert l.og_jpeg_tables_host(75, 8, 8, ql, qc, hdr, 1024, size + off) == OG_EINVAL
    assert l.og_jpeg_coefficients_host(frame, 8, 8, 75, out + 1) == OG_EINVAL and b"aligned to 2" in l.og_last_error()
    assert l.og_jpeg_coefficients_host(None, 8, 8, 75, out) == OG_EINVAL and l.og_jpeg_coefficients_host(frame, 8, 8, 75, None) == OG_EINVAL
    assert l.og_jpeg_tables_host(75, 8, 8, None, qc, hdr, 1024, size) == OG_EINVAL
    assert l.og_jpeg_tables_host(75, 8, 8, ql, None, hdr, 1024, size) == OG_EINVAL
    assert l.og_jpeg_tables_host(75, 8, 8, ql, qc, hdr, 628, size) == OG_EINVAL and b"header_cap" in l.og_last_error()
    assert np.array_equal(buf.snapshot(), before)
    assert l.og_jpeg_encode_host(frame + 1, 8, 8, 75, out + 3, cap, size) == 0       # u8 buffers: any address
    assert l.og_jpeg_tables_host(75, 8, 8, ql + 1, qc + 3, None, 0, None) == 0       # header and its length are optional


def test_host_entries_stay_inside_their_extents():
    for cid in ("1x1-noise-q100", "13x21-noise-q100", "ragged-noise-q50", "ri+1-overlay"):
        c = MC.BY_ID[cid]
        f = c.frames[0]
        H, W = f.shape[:2]
        M = ((H + 7) // 8) * ((W + 7) // 8)
        out = G.run_guarded("og_jpeg_coefficients_host", cid, lambda p: lib().og_jpeg_coefficients_host(p["frame"], H, W, c.quality, p["out"]),
                            {"frame": f}, {"out": M * 192 * 2})
        assert np.array_equal(out["out"].view(np.int16).reshape(M, 3, 64), MJ.coefficients_host(f, c.quality))
        out = G.run_guarded("og_jpeg_tables_host", cid,
                            lambda p: lib().og_jpeg_tables_host(c.quality, H, W, p["ql"], p["qc"], p["hdr"], 629, p["n"]), {},
                            {"ql": 64, "qc": 64, "hdr": 629, "n": 4})
        assert out["hdr"].tobytes() == MC.host_files(cid)[0][:629] and out["n"].view(np.int32)[0] == 629
        # the file: `size` bytes and not one more, at a capacity of exactly the bound
        cap = MJ.bound(H, W)
        want = MC.host_files(cid)[0]
        for slack in (0x00, 0xFF):
            rc, pay, faults = G.guarded_call(lambda p: lib().og_jpeg_encode_host(p["frame"], H, W, c.quality, p["out"], cap, p["size"]),
                                             {"frame": f}, {"out": cap, "size": 4}, slack=slack)
            assert rc == 0 and not faults, (cid, faults)
            n = int(pay["size"].view(np.int32)[0])
            assert pay["out"][:n].tobytes() == want and (pay["out"][n:] == G.GUARD_FILL).all(), cid


def test_the_mjpeg_sources_hold_no_inline_assembly():
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_mjpeg.inc")).read()
    assert "asm" not in src and all(k in src for k in ("k_mjpeg_transform", "k_mjpeg_entropy", "k_mjpeg_offsets", "k_mjpeg_place"))
    assert "while" not in src                                             # every loop is a for over a shape
