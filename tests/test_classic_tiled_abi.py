"""The rules tests/test_classic_abi.py holds the third header to, on the fifth, include/openglottal_hip_classic_tiled.h: every function
it declares is exported and bound (`_lib.TILED_PROTOTYPES`) and vice versa, the table is disjoint from the four older ones, the mode
switch and the new limit are argument checks that come before the first HIP call, and og_blobs_host_any is og_blobs_host without its
limit.  No GPU."""
import os
import re

import numpy as np
import pytest

import buffer_guard as G
import classic_cases as K
from openglottal_amd import _lib
from openglottal_amd import classic as CL
from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL, OG_ESTATE = -1, -2
HEADER = "openglottal_hip_classic_tiled.h"


def _declarations(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_function_of_the_tiled_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == {"og_classic_set_tiled", "og_classic_tiled_limit", "og_blobs_host_any", "og_classic_plan_tiled"}
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        assert getattr(l, name).argtypes == _lib.TILED_PROTOTYPES[name][1]
        assert len(_lib.TILED_PROTOTYPES[name][1]) == len(decl[name]), name
    assert set(decl) == set(_lib.TILED_PROTOTYPES)
    older = set(_lib.PROTOTYPES) | set(_lib.CROP_PROTOTYPES) | set(_lib.CLASSIC_PROTOTYPES) | set(_lib.GATED_PROTOTYPES)
    assert not (set(_lib.TILED_PROTOTYPES) & older)
    assert '#include "openglottal_hip_classic.h"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert len(_lib.PROTOTYPES) == 66 and len(_lib.CROP_PROTOTYPES) == 7 and len(_lib.CLASSIC_PROTOTYPES) == 20 and len(_lib.GATED_PROTOTYPES) == 13


def test_limits():
    l = lib()
    limit, T = l.og_classic_tiled_limit(0), l.og_classic_tiled_limit(1)
    assert limit >= 480 * 640 and T >= 8 and l.og_classic_tiled_limit(2) == -1 and l.og_classic_tiled_limit(-1) == -1
    assert l.og_classic_limit(0) == 65536                                 # the old limit stays


def test_the_mode_switch_and_the_new_limit_without_a_device():
    l = lib()
    h = l.og_classic_create()
    assert h
    try:
        raw = np.zeros(4096, np.uint8)
        base = raw.ctypes.data + (-raw.ctypes.data) % 8
        frames, boxes, area = base, base + 1024, base + 2048
        assert l.og_classic_set_tiled(h, 3) == OG_EINVAL and l.og_classic_set_tiled(h, -1) == OG_EINVAL
        assert l.og_classic_set_tiled(None, 1) == OG_EINVAL
        assert l.og_vft_guided_stream_u8(h, frames, 1, 257, 256, 1, boxes, None, area, None) == OG_EINVAL      # the default is off
        assert b"65536" in l.og_last_error()
        limit = l.og_classic_tiled_limit(0)
        for mode in (1, 2):
            assert l.og_classic_set_tiled(h, mode) == 0
            assert l.og_vft_guided_stream_u8(h, frames, 1, 257, 256, 1, boxes, None, area, None) == OG_ESTATE  # accepted: no threshold yet
            assert l.og_vft_guided_u8_dev(h, frames, 1, 480, 640, 3, boxes, None, area, None) == OG_ESTATE
            assert l.og_vft_guided_stream_u8(h, frames, 1, 257, 256, 1, boxes + 2, None, area, None) == OG_EINVAL   # alignment rules unchanged
            assert l.og_otsu_in_box_u8(h, frames, 0, 480, 640, 1, boxes, None, area, area) == 0                # B = 0: nothing to do
            for fn in (l.og_vft_guided_stream_u8, l.og_vft_guided_u8_dev, l.og_otsu_in_box_u8, l.og_otsu_in_box_u8_dev):
                assert fn(h, frames, 1, 1, limit + 1, 1, boxes, None, area, area) == OG_EINVAL                 # one pixel above
                assert str(limit).encode() in l.og_last_error()
            assert l.og_vft_guided_init_u8(h, frames, 1, 1, limit + 1, 1, None, None) == OG_EINVAL
            assert str(limit).encode() in l.og_last_error()
        assert l.og_classic_set_tiled(h, 0) == 0
        assert l.og_vft_guided_stream_u8(h, frames, 1, 257, 256, 1, boxes, None, area, None) == OG_EINVAL
        assert b"65536" in l.og_last_error()
        assert l.og_classic_sync(h) == 0 and not raw.any()                # nothing touched a device or a buffer
    finally:
        l.og_classic_destroy(h)
    with pytest.raises(CL.OpenGlottalHipError):
        CL.Classic(tiled="sometimes")
    assert CL.Classic().tiled == "off" and CL.Classic(tiled="auto").tiled == "auto"


def test_blobs_host_any_equals_scipy_above_the_old_limit():
    for name, m in K.hard_masks(257):
        assert m.size > lib().og_classic_limit(0)
        for want_mask in (True, False):
            out, area = CL.blobs_host(m, 2, want_mask)                    # goes to og_blobs_host_any above the old limit
            s_out, s_area = K.scipy_blobs_cached(m, 2)
            assert area == s_area and (out is None or np.array_equal(out, s_out)), name
    rs = np.random.RandomState(5)
    canvas = (rs.rand(300, 260) < 0.55).astype(np.uint8)
    hard = dict(K.hard_masks(160))
    canvas[20:180, 30:190] |= hard["rings"]
    canvas[120:280, 80:240] ^= hard["spiral"]
    for n in K.NS:
        out, area = CL.blobs_host(canvas, n)
        s_out, s_area = K.scipy_blobs(canvas, n)
        assert area == s_area and np.array_equal(out, s_out), n
    area = np.zeros(1, np.int32)
    big = np.zeros((257, 256), np.uint8)
    assert lib().og_blobs_host(big.ctypes.data, 257, 256, 2, None, area.ctypes.data) == OG_EINVAL      # the old entry keeps its check


def test_blobs_host_any_equals_blobs_host_below_the_old_limit():
    l = lib()
    cases = list(K.named_masks()) + [(f"{k}-{S}", m) for S in (33, 64, 96) for k, m in K.hard_masks(S)]
    for name, m in cases:
        assert m.shape[0] <= 96 and m.shape[1] <= 96
        for n in (1, 2, 8):
            a, b = np.full(m.shape, 7, np.uint8), np.full(m.shape, 9, np.uint8)
            aa, ab = np.zeros(1, np.int32), np.zeros(1, np.int32)
            assert l.og_blobs_host(m.ctypes.data, m.shape[0], m.shape[1], n, a.ctypes.data, aa.ctypes.data) == 0
            assert l.og_blobs_host_any(m.ctypes.data, m.shape[0], m.shape[1], n, b.ctypes.data, ab.ctypes.data) == 0
            assert aa[0] == ab[0] and np.array_equal(a, b), (name, n)


def test_blobs_host_any_stays_inside_its_extents_and_refuses_a_misaligned_area():
    m = dict(K.hard_masks(257))["rings"]
    for want_mask in (True, False):
        out = G.run_guarded("og_blobs_host_any", f"rings 257 mask={want_mask}",
                            lambda p: lib().og_blobs_host_any(p["mask"], 257, 257, 2, p["out"], p["area"]),
                            {"mask": m}, {"out": m.size if want_mask else None, "area": 4})
        assert out["area"].view(np.int32)[0] == K.scipy_blobs_cached(m, 2)[1]
    buf = G.Region("b", 1 << 16, "host", G.guard_bytes(1 << 16), G.GUARD_FILL)
    a = buf.ptr
    before = buf.snapshot()
    l = lib()
    for off in (1, 2, 3):
        assert l.og_blobs_host_any(a + 16384, 8, 8, 2, a + 16384 + 64, a + 2048 + off) == OG_EINVAL
    assert l.og_blobs_host_any(a + 16384, 8, 8, 0, a + 16384 + 64, a + 2048) == OG_EINVAL
    assert l.og_blobs_host_any(a + 16384, 0, 8, 2, a + 16384 + 64, a + 2048) == OG_EINVAL
    assert np.array_equal(buf.snapshot(), before)
    assert l.og_blobs_host_any(a + 16385, 8, 8, 2, a + 16384 + 67, a + 2048) == 0                        # u8 buffers: any address


def test_the_tiled_kernels_hold_no_inline_assembly():
    kern = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_kernels.hpp")).read()
    new = kern[kern.index("the tiled blob filter"):kern.index("The temporal tracker of the gated pipeline")]
    assert "asm" not in new and "k_tblob_paint" in new
