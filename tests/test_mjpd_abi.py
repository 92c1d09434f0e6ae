"""The rules tests/test_mjpeg_abi.py holds the ninth header to, on the tenth, include/decode/openglottal_hip_mjpd.h: every function it
declares is exported and bound (`_lib.MJPD_PROTOTYPES`) and vice versa, the table is disjoint from the nine older ones and those are
untouched, every argument check comes before the first HIP call, and B = 0 is a no-op.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import mjpd_cases as DC
from openglottal_amd import _lib
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL, OG_ESTATE = -1, -2
HEADER = os.path.join(ROOT, "include", "decode", "openglottal_hip_mjpd.h")
OLDER = {"openglottal_hip.h": ("PROTOTYPES", 66), "openglottal_hip_crops.h": ("CROP_PROTOTYPES", 7),
         "openglottal_hip_classic.h": ("CLASSIC_PROTOTYPES", 20), "openglottal_hip_gated.h": ("GATED_PROTOTYPES", 13),
         "openglottal_hip_classic_tiled.h": ("TILED_PROTOTYPES", 4), "openglottal_hip_overlay.h": ("OVERLAY_PROTOTYPES", 11),
         "openglottal_hip_sweep.h": ("SWEEP_PROTOTYPES", 11), "openglottal_hip_gate.h": ("GATE_PROTOTYPES", 8),
         "openglottal_hip_mjpeg.h": ("MJPEG_PROTOTYPES", 13)}


def _declarations(path):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_function_of_the_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == {"og_mjpd_limit", "og_jpegd_parse_host", "og_jpegd_decode_host", "og_jpegd_records_host", "og_jpegd_idct_pass_host", "og_mjpd_create",
                         "og_mjpd_destroy", "og_mjpd_sync", "og_mjpd_set_chunk", "og_mjpd_set_tables", "og_mjpd_decode_u8_dev",
                         "og_mjpd_decode_stream", "og_mjpd_plan"}
    assert all(n.startswith(("og_mjpd_", "og_jpegd_")) for n in decl)
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        args = _lib.MJPD_PROTOTYPES[name][1]
        assert list(getattr(l, name).argtypes or []) == args, name
        assert len(args) == (0 if decl[name] == ["void"] else len(decl[name])), name
    assert set(decl) == set(_lib.MJPD_PROTOTYPES)
    text = open(HEADER).read()
    assert '#include "../openglottal_hip.h"' in text and "UNPINNED" in text


def test_the_nine_older_headers_and_tables_are_untouched():
    seen = set()
    for header, (table, count) in OLDER.items():
        t = getattr(_lib, table)
        assert len(t) == count and set(_declarations(os.path.join(ROOT, "include", header))) == set(t), header
        assert not (set(t) & set(_lib.MJPD_PROTOTYPES)) and not (set(t) & seen), header
        seen |= set(t)
    assert len([f for f in os.listdir(os.path.join(ROOT, "include")) if f.endswith(".h")]) == 9
    assert os.listdir(os.path.join(ROOT, "include", "decode")) == ["openglottal_hip_mjpd.h"]
    api = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_api.hip")).read()
    assert api.count('#include "og_mjpd.inc"') == 1 and api.index('#include "og_mjpeg.inc"') < api.index('#include "og_mjpd.inc"')


def test_limits_and_layouts():
    l = lib()
    assert [l.og_mjpd_limit(i) for i in range(7)] == [l.og_mjpeg_limit(0), 1024, 32, 6120, 7, 1 << 30, 128]
    assert l.og_mjpd_limit(7) == -1 and l.og_mjpd_limit(-1) == -1
    assert C.sizeof(MJ._Info) == 56 and set(MJ.STATUS) == set(range(8))
    e = MJ.MjpegDecoder()
    assert e.chunk == 128


def test_the_handle_refuses_bad_arguments_without_a_device():
    """Argument checks come before the first HIP call, so they can be held here."""
    l = lib()
    h = l.og_mjpd_create()
    assert h
    try:
        raw = np.zeros(1 << 16, np.uint8)
        base = raw.ctypes.data + (-raw.ctypes.data) % 8
        blob, offsets, recs, frames, status, hw = base, base + 8192, base + 16384, base + 24576, base + 32768, base + 40960
        j = DC.pillow_jpeg(8, 8, "444")
        raw[:len(j)] = np.frombuffer(j, np.uint8)
        np.frombuffer(raw, np.int64, 2, offsets - raw.ctypes.data)[:] = (0, len(j))
        before = raw.copy()
        cap = 8 * 8 * 3
        dev, stream = l.og_mjpd_decode_u8_dev, l.og_mjpd_decode_stream
        assert dev(None, blob, offsets, recs, 1, 8, 8, frames, cap, status) == OG_EINVAL and b"null handle" in l.og_last_error()
        assert stream(None, blob, offsets, 1, frames, None, cap, status, hw, hw + 4) == OG_EINVAL and b"null handle" in l.og_last_error()
        assert dev(h, blob, offsets, recs, 1, 8, 8, frames, cap - 1, status) == OG_EINVAL and b"cap is below" in l.og_last_error()
        assert dev(h, blob, offsets, recs, 3, 8, 8, frames, 3 * cap - 1, status) == OG_EINVAL
        assert stream(h, blob, offsets, 1, frames, None, cap - 1, status, hw, hw + 4) == OG_EINVAL and b"cap is below" in l.og_last_error()
        assert str(cap).encode() in l.og_last_error()
        assert dev(h, blob, offsets, recs, -1, 8, 8, frames, cap, status) == OG_EINVAL
        assert dev(h, blob, offsets, recs, 1, 0, 8, frames, cap, status) == OG_EINVAL
        assert dev(h, blob, offsets, recs, 1, 1, l.og_mjpd_limit(0) + 1, frames, 1 << 40, status) == OG_EINVAL
        for off in (1, 2, 4, 7):
            assert dev(h, blob, offsets + off, recs, 1, 8, 8, frames, cap, status) == OG_EINVAL and b"aligned to 8" in l.og_last_error()
            assert stream(h, blob, offsets + off, 1, frames, None, cap, status, hw, hw + 4) == OG_EINVAL and b"aligned to 8" in l.og_last_error()
        for off in (1, 2, 3):
            assert dev(h, blob, offsets, recs + off, 1, 8, 8, frames, cap, status) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
            assert dev(h, blob, offsets, recs, 1, 8, 8, frames, cap, status + off) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
            assert stream(h, blob, offsets, 1, frames, None, cap, status + off, hw, hw + 4) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
            assert stream(h, blob, offsets, 1, frames, None, cap, status, hw + off, hw + 4) == OG_EINVAL
        for i in range(1, 5):
            args = [blob, offsets, recs, 1, 8, 8, frames, cap, status]
            args[{1: 0, 2: 1, 3: 2, 4: 6}[i]] = None
            assert dev(h, *args) == OG_EINVAL
        assert dev(h, blob, offsets, recs, 1, 8, 8, frames, cap, status) == OG_ESTATE and b"og_mjpd_set_tables" in l.og_last_error()
        assert stream(h, None, offsets, 1, frames, None, cap, status, hw, hw + 4) == OG_EINVAL
        assert stream(h, blob, None, 1, frames, None, cap, status, hw, hw + 4) == OG_EINVAL
        assert stream(h, blob, offsets, 1, None, None, cap, status, hw, hw + 4) == OG_EINVAL and b"no place" in l.og_last_error()
        assert stream(h, blob, offsets, 1, frames, None, cap, None, hw, hw + 4) == OG_EINVAL
        assert stream(h, blob, offsets, 1, frames, None, cap, status, None, hw + 4) == OG_EINVAL
        assert l.og_mjpd_set_tables(h, None, 1, 1, 0) == OG_EINVAL and l.og_mjpd_set_tables(h, blob, 0, 1, 0) == OG_EINVAL
        assert l.og_mjpd_set_tables(h, blob, 1, 4, 0) == OG_EINVAL and l.og_mjpd_set_tables(h, blob, 1, 1, -1) == OG_EINVAL
        assert l.og_mjpd_set_tables(h, blob + 2, 1, 1, 0) == OG_EINVAL and l.og_mjpd_set_tables(None, blob, 1, 1, 0) == OG_EINVAL
        # B = 0: nothing to do
        assert dev(h, blob, offsets, recs, 0, 8, 8, frames, 0, status) == 0
        assert stream(h, blob, offsets, 0, frames, None, 0, status, hw, hw + 4) == 0
        assert np.array_equal(raw, before)                                    # nothing touched a device or a buffer
        # every file refused by the parser: the statuses, and still no device
        np.frombuffer(raw, np.uint8, 2, 0)[:] = 0
        assert stream(h, blob, offsets, 1, frames, None, cap, status, hw, hw + 4) == 0
        assert np.frombuffer(raw, np.int32, 1, status - raw.ctypes.data)[0] == 6 and b"no SOI" in l.og_last_error()
        assert l.og_mjpd_set_chunk(h, 0) == OG_EINVAL and l.og_mjpd_set_chunk(h, 1025) == OG_EINVAL and l.og_mjpd_set_chunk(h, 7) == 0
        assert l.og_mjpd_set_chunk(None, 4) == OG_EINVAL and l.og_mjpd_sync(None) == OG_EINVAL
        assert l.og_mjpd_sync(h) == 0                                         # no stream yet: nothing to wait for
    finally:
        l.og_mjpd_destroy(h)
    l.og_mjpd_destroy(None)


def test_the_host_entries_refuse_bad_arguments():
    l = lib()
    j = np.frombuffer(DC.pillow_jpeg(8, 8, "444"), np.uint8)
    out, st, info = np.zeros(256, np.uint8), np.zeros(2, np.int32), np.zeros(64, np.uint8)
    assert l.og_jpegd_decode_host(j.ctypes.data, j.size, out.ctypes.data, 191, st.ctypes.data) == OG_EINVAL and b"cap is below" in l.og_last_error()
    assert not out.any()
    assert l.og_jpegd_decode_host(None, j.size, out.ctypes.data, 192, st.ctypes.data) == OG_EINVAL
    assert l.og_jpegd_decode_host(j.ctypes.data, j.size, None, 192, st.ctypes.data) == OG_EINVAL
    assert l.og_jpegd_decode_host(j.ctypes.data, j.size, out.ctypes.data, 192, None) == OG_EINVAL
    assert l.og_jpegd_decode_host(j.ctypes.data, j.size, out.ctypes.data, 192, st.ctypes.data + 2) == OG_EINVAL
    assert l.og_jpegd_parse_host(None, 4, info.ctypes.data) == OG_EINVAL and l.og_jpegd_parse_host(j.ctypes.data, j.size, None) == OG_EINVAL
    assert l.og_jpegd_parse_host(j.ctypes.data, j.size, info.ctypes.data + 4) == OG_EINVAL
    assert l.og_jpegd_decode_host(j.ctypes.data, j.size, out.ctypes.data, 192, st.ctypes.data) == 0 and st[0] == 0 and out[:192].any()


def test_records_and_table_sets():
    a, b = DC.pillow_jpeg(17, 9, "420", 75, 1), DC.pillow_jpeg(17, 9, "420", 30, 1, True)
    blob, offsets, recs, tabs, form = MJ.records_host([a, b, a, DC.pillow_jpeg(17, 9, "420", 75, 3), DC.pillow_jpeg(17, 9, "444", 75, 1), b"junk"])
    assert form == {"H": 17, "W": 9, "sampling": 3, "Ri": 1} and tabs.shape == (2, 6120)
    assert recs[:, 2].tolist() == [0, 0, 0, 7, 7, 6] and recs[:3, 3].tolist() == [0, 1, 0]
    info = MJ.parse(a)
    assert recs[0].tolist() == [info["scan_offset"], info["scan_length"], 0, 0, 1, info["nI"], 0, 0]


def test_the_decoder_sources_hold_no_inline_assembly():
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_mjpd.inc")).read()
    assert "asm" not in src and all(k in src for k in ("k_mjpd_markers", "k_mjpd_entropy", "k_mjpd_idct", "k_mjpd_colour"))
    assert "og_jpeg_annexk.inc" in open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_mjpeg.inc")).read()      # the shared Annex K tables
