"""The rules tests/test_mjps_abi.py holds the eleventh header to, on the twelfth, include_ext/openglottal_hip_png.h: every function it
declares is exported and bound (`_lib.PNG_PROTOTYPES`) and vice versa, the table is disjoint from the eleven older ones and those are
untouched, every argument and alignment check comes before the first HIP call, and B = 0 is a no-op.  No GPU."""
import ctypes as C
import os

import numpy as np

import png_cases as PC
from openglottal_amd import _lib
from openglottal_amd import png as P
from openglottal_amd._lib import lib
from test_mjpd_abi import OLDER, ROOT, _declarations

OG_EINVAL, OG_ESTATE = -1, -2
HEADER = os.path.join(ROOT, "include_ext", "openglottal_hip_png.h")
NAMES = {"og_png_limit", "og_pngd_parse_host", "og_pngd_inflate_host", "og_pngd_decode_host", "og_pngd_records_host", "og_png_create",
         "og_png_destroy", "og_png_sync", "og_png_set_chunk", "og_png_set_palettes", "og_png_decode_u8_dev", "og_png_decode_stream", "og_png_plan"}


def test_every_function_of_the_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == NAMES == set(_lib.PNG_PROTOTYPES)
    assert all(n.startswith(("og_png_", "og_pngd_")) for n in decl)
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        args = _lib.PNG_PROTOTYPES[name][1]
        assert list(getattr(l, name).argtypes or []) == args, name
        assert len(args) == (0 if decl[name] == ["void"] else len(decl[name])), name
    text = open(HEADER).read()
    assert '#include "../include/openglottal_hip.h"' in text and "UNPINNED" in text and "SAFETY" in text


def test_the_eleven_older_headers_and_tables_are_untouched():
    seen = set(_lib.PNG_PROTOTYPES)
    older = dict(OLDER, **{"decode/openglottal_hip_mjpd.h": ("MJPD_PROTOTYPES", 13), "split/openglottal_hip_mjps.h": ("MJPS_PROTOTYPES", 4)})
    for header, (table, count) in older.items():
        t = getattr(_lib, table)
        assert len(t) == count and set(_declarations(os.path.join(ROOT, "include", header))) == set(t), header
        assert not (set(t) & seen), header
        seen |= set(t)
    assert os.listdir(os.path.join(ROOT, "include_ext")) == ["openglottal_hip_png.h"]
    api = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_api.hip")).read()
    assert api.count('#include "og_png.inc"') == 1 and api.index('#include "og_mjps.inc"') < api.index('#include "og_png.inc"')
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_png.inc")).read()
    assert "asm" not in src and all(k in src for k in ("k_png_inflate", "k_png_unfilter", "k_png_expand", "OG_PNG_HOST_ONLY"))
    assert "include_ext" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_limits_and_layouts():
    l = lib()
    assert [l.og_png_limit(i) for i in range(8)] == [l.og_mjpd_limit(0), 1024, 40, 768, 7, 1 << 30, 128, 32768]
    assert l.og_png_limit(8) == -1 and l.og_png_limit(-1) == -1
    assert C.sizeof(P._Info) == 56 and P.REC.itemsize == 40 and set(P.STATUS) == set(range(8))
    assert P.PngDecoder().chunk == 128


def test_the_handle_refuses_bad_arguments_without_a_device():
    """Argument checks come before the first HIP call, so they can be held here."""
    l = lib()
    h = l.og_png_create()
    assert h
    try:
        raw = np.zeros(1 << 16, np.uint8)
        base = raw.ctypes.data + (-raw.ctypes.data) % 8
        blob, offsets, recs, out, status, oo, hw = (base + 8192 * i for i in range(7))
        f = PC.simple(4, 6, 0, 8, None, 1)
        raw[blob - raw.ctypes.data:blob - raw.ctypes.data + len(f)] = np.frombuffer(f, np.uint8)
        np.frombuffer(raw, np.int64, 2, offsets - raw.ctypes.data)[:] = (0, len(f))
        before = raw.copy()
        cap = 4 * 6 * 3
        dev, stream = l.og_png_decode_u8_dev, l.og_png_decode_stream
        assert dev(None, blob, offsets, recs, 1, 3, 28, 24, out, cap, status) == OG_EINVAL and b"null handle" in l.og_last_error()
        assert stream(None, blob, offsets, 1, 3, out, None, cap, oo, hw, status) == OG_EINVAL and b"null handle" in l.og_last_error()
        assert stream(h, blob, offsets, 1, 3, out, None, cap - 1, oo, hw, status) == OG_EINVAL and b"cap is below" in l.og_last_error()
        assert str(cap).encode() in l.og_last_error()
        assert stream(h, blob, offsets, 1, 1, out, None, 23, oo, hw, status) == OG_EINVAL
        for ch in (0, 2, 4):
            assert stream(h, blob, offsets, 1, ch, out, None, cap, oo, hw, status) == OG_EINVAL and b"channels" in l.og_last_error()
            assert dev(h, blob, offsets, recs, 1, ch, 28, 24, out, cap, status) == OG_EINVAL and b"channels" in l.og_last_error()
        assert dev(h, blob, offsets, recs, -1, 3, 28, 24, out, cap, status) == OG_EINVAL
        assert dev(h, blob, offsets, recs, 1, 3, -1, 24, out, cap, status) == OG_EINVAL
        assert dev(h, blob, offsets, recs, 1, 3, 28, 0, out, cap, status) == OG_EINVAL
        assert dev(h, blob, offsets, recs, 1, 3, 28, l.og_png_limit(0) + 1, out, cap, status) == OG_EINVAL
        for off in (1, 2, 4, 7):
            assert dev(h, blob, offsets + off, recs, 1, 3, 28, 24, out, cap, status) == OG_EINVAL and b"aligned to 8" in l.og_last_error()
            assert dev(h, blob, offsets, recs + off, 1, 3, 28, 24, out, cap, status) == OG_EINVAL and b"aligned to 8" in l.og_last_error()
            assert stream(h, blob, offsets + off, 1, 3, out, None, cap, oo, hw, status) == OG_EINVAL and b"aligned to 8" in l.og_last_error()
            assert stream(h, blob, offsets, 1, 3, out, None, cap, oo + off, hw, status) == OG_EINVAL and b"aligned to 8" in l.og_last_error()
        for off in (1, 2, 3):
            assert dev(h, blob, offsets, recs, 1, 3, 28, 24, out, cap, status + off) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
            assert stream(h, blob, offsets, 1, 3, out, None, cap, oo, hw, status + off) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
            assert stream(h, blob, offsets, 1, 3, out, None, cap, oo, hw + off, status) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
        for i in (0, 1, 2, 7, 9):
            args = [blob, offsets, recs, 1, 3, 28, 24, out, cap, status]
            args[i] = None
            assert dev(h, *args) == OG_EINVAL
        assert dev(h, blob, offsets, recs, 1, 3, 28, 24, out, cap, status) == OG_ESTATE and b"og_png_set_palettes" in l.og_last_error()
        assert stream(h, None, offsets, 1, 3, out, None, cap, oo, hw, status) == OG_EINVAL
        assert stream(h, blob, None, 1, 3, out, None, cap, oo, hw, status) == OG_EINVAL
        assert stream(h, blob, offsets, 1, 3, None, None, cap, oo, hw, status) == OG_EINVAL and b"no place" in l.og_last_error()
        assert stream(h, blob, offsets, 1, 3, out, None, cap, None, hw, status) == OG_EINVAL
        assert stream(h, blob, offsets, 1, 3, out, None, cap, oo, None, status) == OG_EINVAL
        assert stream(h, blob, offsets, 1, 3, out, None, cap, oo, hw, None) == OG_EINVAL
        assert l.og_png_set_palettes(None, blob, 1) == OG_EINVAL and l.og_png_set_palettes(h, None, 1) == OG_EINVAL
        assert l.og_png_set_palettes(h, blob, -1) == OG_EINVAL and l.og_png_set_palettes(h, blob, 65536) == OG_EINVAL
        # B = 0: nothing to do
        assert dev(h, blob, offsets, recs, 0, 3, 0, 1, out, 0, status) == 0
        raw[oo - raw.ctypes.data] = 9
        assert stream(h, blob, offsets, 0, 3, out, None, 0, oo, hw, status) == 0 and raw[oo - raw.ctypes.data] == 0
        assert np.array_equal(raw, before)                                    # nothing touched a device or a buffer
        # every file refused by the parser: the statuses, and still no device
        raw[blob - raw.ctypes.data] = 0
        assert stream(h, blob, offsets, 1, 3, out, None, cap, oo, hw, status) == 0
        assert np.frombuffer(raw, np.int32, 1, status - raw.ctypes.data)[0] == 6 and b"no PNG signature" in l.og_last_error()
        assert np.frombuffer(raw, np.int64, 2, oo - raw.ctypes.data).tolist() == [0, 0]
        assert l.og_png_set_chunk(h, 0) == OG_EINVAL and l.og_png_set_chunk(h, 1025) == OG_EINVAL and l.og_png_set_chunk(h, 7) == 0
        assert l.og_png_set_chunk(None, 4) == OG_EINVAL and l.og_png_sync(None) == OG_EINVAL
        assert l.og_png_sync(h) == 0                                          # no stream yet: nothing to wait for
    finally:
        l.og_png_destroy(h)
    l.og_png_destroy(None)


def test_the_host_entries_refuse_bad_arguments():
    l = lib()
    f = np.frombuffer(PC.simple(4, 6, 0, 8, None, 1), np.uint8)
    out, st, info = np.zeros(256, np.uint8), np.zeros(4, np.int32), np.zeros(64, np.uint8)
    dec = l.og_pngd_decode_host
    assert dec(f.ctypes.data, f.size, 3, out.ctypes.data, 71, st.ctypes.data) == OG_EINVAL and b"cap is below" in l.og_last_error()
    assert dec(f.ctypes.data, f.size, 2, out.ctypes.data, 72, st.ctypes.data) == OG_EINVAL
    assert dec(None, f.size, 3, out.ctypes.data, 72, st.ctypes.data) == OG_EINVAL and dec(f.ctypes.data, f.size, 3, None, 72, st.ctypes.data) == OG_EINVAL
    assert dec(f.ctypes.data, f.size, 3, out.ctypes.data, 72, None) == OG_EINVAL
    assert dec(f.ctypes.data, f.size, 3, out.ctypes.data, 72, st.ctypes.data + 2) == OG_EINVAL
    assert not out.any()
    assert l.og_pngd_parse_host(None, 4, info.ctypes.data) == OG_EINVAL and l.og_pngd_parse_host(f.ctypes.data, f.size, None) == OG_EINVAL
    assert l.og_pngd_parse_host(f.ctypes.data, f.size, info.ctypes.data + 4) == OG_EINVAL
    n = np.zeros(2, np.uint64)
    inf = l.og_pngd_inflate_host
    assert inf(None, 4, out.ctypes.data, 8, n.ctypes.data, st.ctypes.data) == OG_EINVAL and inf(f.ctypes.data, 4, None, 8, n.ctypes.data, st.ctypes.data) == OG_EINVAL
    assert inf(f.ctypes.data, 4, out.ctypes.data, 8, n.ctypes.data + 4, st.ctypes.data) == OG_EINVAL
    assert inf(f.ctypes.data, 4, out.ctypes.data, 8, n.ctypes.data, st.ctypes.data + 1) == OG_EINVAL
    assert dec(f.ctypes.data, f.size, 3, out.ctypes.data, 72, st.ctypes.data) == 0 and st[0] == 0 and out[:72].any() and not out[72:].any()


def test_records_palettes_and_dense_offsets():
    pal = PC.palette(4, 1)
    files = [PC.simple(4, 6, 0, 8, None, 1), PC.simple(3, 5, 3, 2, None, 2, plte=pal), b"junk", PC.simple(2, 2, 3, 4, None, 3),
             PC.simple(3, 5, 3, 2, None, 4, plte=pal, idat=1)]
    r = P.records_host(files, 3)
    recs = r["recs"]
    assert recs["status"].tolist() == [0, 0, 6, 0, 0] and recs["palette"].tolist() == [0, 0, 0, 1, 0] and r["pals"].shape == (2, 768)
    assert recs["out_offset"].tolist() == [0, 72, 117, 117, 129] and r["out_bytes"] == 129 + 45 and r["max_pixels"] == 24
    assert recs["raw_offset"].tolist() == [0, 28, 37, 37, 41] and r["raw_bytes"] == 41 + 9
    assert [int(b - a) for a, b in zip(r["zoffsets"], r["zoffsets"][1:])] == [P.parse(f).get("zlib_bytes", 0) if f != b"junk" else 0 for f in files]
    z = r["zblob"][int(r["zoffsets"][4]):int(r["zoffsets"][5])].tobytes()
    assert z == PC.stream_of(files[4])                                       # the IDAT payloads joined: no chunk header inside
    assert P.records_host(files, 1)["out_bytes"] == (129 + 45) // 3
