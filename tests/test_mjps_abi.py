"""The rules tests/test_mjpd_abi.py holds the tenth header to, on the eleventh, include/split/openglottal_hip_mjps.h: every function it
declares is exported and bound (`_lib.MJPS_PROTOTYPES`) and vice versa, the table is disjoint from the ten older ones and those are
untouched, every argument check comes before the first HIP call, and the mode is off unless it is asked for.  No GPU."""
import os

import numpy as np

import mjpd_cases as DC
from openglottal_amd import _lib
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import lib
from test_mjpd_abi import OLDER, ROOT, _declarations

OG_EINVAL, OG_ESTATE = -1, -2
HEADER = os.path.join(ROOT, "include", "split", "openglottal_hip_mjps.h")
NAMES = {"og_mjps_limit", "og_mjps_set_split", "og_mjps_plan", "og_jpegs_decode_host"}


def test_every_function_of_the_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == NAMES == set(_lib.MJPS_PROTOTYPES)
    assert all(n.startswith(("og_mjps_", "og_jpegs_")) for n in decl)
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        args = _lib.MJPS_PROTOTYPES[name][1]
        assert list(getattr(l, name).argtypes or []) == args, name
        assert len(args) == len(decl[name]), name
    text = open(HEADER).read()
    assert '#include "../decode/openglottal_hip_mjpd.h"' in text and "at most (lanes of the window) rounds" in text


def test_the_ten_older_headers_and_tables_are_untouched():
    seen = set(_lib.MJPS_PROTOTYPES)
    older = dict(OLDER, **{"decode/openglottal_hip_mjpd.h": ("MJPD_PROTOTYPES", 13)})
    for header, (table, count) in older.items():
        t = getattr(_lib, table)
        assert len(t) == count and set(_declarations(os.path.join(ROOT, "include", header))) == set(t), header
        assert not (set(t) & seen), header
        seen |= set(t)
    assert os.listdir(os.path.join(ROOT, "include", "split")) == ["openglottal_hip_mjps.h"]
    assert sorted(d for d in os.listdir(os.path.join(ROOT, "include")) if not d.endswith(".h")) == ["decode", "split"]
    api = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_api.hip")).read()
    assert api.count('#include "og_mjps.inc"') == 1 and api.index('#include "og_mjpd.inc"') < api.index('#include "og_mjps.inc"')
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_mjps.inc")).read()
    assert "asm" not in src and "k_mjps_entropy" in src and "__syncthreads_or" in src and "OG_MJPD_HOST_ONLY" in src


def test_set_split_refuses_bad_arguments_without_a_device_and_is_off_by_default():
    l = lib()
    h = l.og_mjpd_create()
    assert h
    try:
        assert l.og_mjps_set_split(None, 0, 0) == OG_EINVAL and b"null handle" in l.og_last_error()
        for mode in (-1, 2, 7):
            assert l.og_mjps_set_split(h, mode, 0) == OG_EINVAL and b"mode" in l.og_last_error()
        for sub in (-4, 1, 2, 3, 6, 1022, 1028, 4096):
            assert l.og_mjps_set_split(h, 1, sub) == OG_EINVAL and b"sub" in l.og_last_error()
            assert l.og_mjps_set_split(h, 0, sub) == OG_EINVAL
        for sub in (0, 4, 8, 64, 1024):
            assert l.og_mjps_set_split(h, 1, sub) == 0 and l.og_mjps_set_split(h, 0, sub) == 0
        assert l.og_mjpd_sync(h) == 0                                         # still no stream: nothing touched a device
        # the checks of the decode entries still come first with the mode on
        assert l.og_mjps_set_split(h, 1, 4) == 0
        raw = np.zeros(1 << 12, np.uint8)
        base = raw.ctypes.data + (-raw.ctypes.data) % 8
        assert l.og_mjpd_decode_u8_dev(h, base, base + 1024, base + 2048, 1, 8, 8, base + 3072, 191, base + 3584) == OG_EINVAL
        assert l.og_mjpd_decode_u8_dev(h, base, base + 1024, base + 2048, 1, 8, 8, base + 3072, 192, base + 3584) == OG_ESTATE
    finally:
        l.og_mjpd_destroy(h)
    d = MJ.MjpegDecoder()
    assert (d.split, d.sub, d.chunk) == ("off", 0, 128)
    d.set_split("auto", 32)
    assert (d.split, d.sub) == ("auto", 32)
    for bad in (("on", None), ("auto", 6)):
        try:
            d.set_split(*bad)
        except _lib.OpenGlottalHipError:
            pass
        else:
            raise AssertionError(bad)
    assert (d.split, d.sub) == ("auto", 32)                                   # a refused call changes nothing


def test_the_twin_refuses_bad_arguments():
    l = lib()
    j = np.frombuffer(DC.pillow_jpeg(8, 8, "444"), np.uint8)
    out, st, stats = np.zeros(256, np.uint8), np.zeros(2, np.int32), np.zeros(5, np.int32)
    call = l.og_jpegs_decode_host
    assert call(j.ctypes.data, j.size, 4, 4, out.ctypes.data, 191, st.ctypes.data, stats.ctypes.data) == OG_EINVAL and b"cap is below" in l.og_last_error()
    assert not out.any()
    assert call(None, j.size, 4, 4, out.ctypes.data, 192, st.ctypes.data, None) == OG_EINVAL
    assert call(j.ctypes.data, j.size, 4, 4, None, 192, st.ctypes.data, None) == OG_EINVAL
    assert call(j.ctypes.data, j.size, 4, 4, out.ctypes.data, 192, None, None) == OG_EINVAL
    assert call(j.ctypes.data, j.size, 4, 4, out.ctypes.data, 192, st.ctypes.data + 2, None) == OG_EINVAL
    assert call(j.ctypes.data, j.size, 4, 4, out.ctypes.data, 192, st.ctypes.data, stats.ctypes.data + 2) == OG_EINVAL
    assert call(j.ctypes.data, j.size, 6, 4, out.ctypes.data, 192, st.ctypes.data, None) == OG_EINVAL
    assert call(j.ctypes.data, j.size, 4, 0, out.ctypes.data, 192, st.ctypes.data, None) == OG_EINVAL
    assert call(j.ctypes.data, j.size, 4, 257, out.ctypes.data, 192, st.ctypes.data, None) == OG_EINVAL
    assert not out.any() and not stats.any()
    assert call(j.ctypes.data, j.size, 4, 4, out.ctypes.data, 192, st.ctypes.data, None) == 0 and st[0] == 0 and out[:192].any()
    assert call(j.ctypes.data, j.size, 4, 4, out.ctypes.data, 192, st.ctypes.data, stats.ctypes.data) == 0 and stats[0] > 0 and stats[4] == 0


def test_cli_flag():
    from openglottal_amd import cli

    text = open(cli.__file__).read()
    assert text.count('"--decode-split"') == 1 and 'choices=["off", "auto"], default="off"' in text
