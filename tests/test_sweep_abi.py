"""The rules tests/test_overlay_abi.py holds the sixth header to, on the seventh, include/openglottal_hip_sweep.h: every function it
declares is exported and bound (`_lib.SWEEP_PROTOTYPES`) and vice versa, the table is disjoint from the six older ones, every
argument check comes before the first HIP call and touches no buffer, and the sources hold no inline assembly.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

from openglottal_amd import _lib, gated
from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL = -1
HEADER = "openglottal_hip_sweep.h"


def _declarations(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_function_of_the_sweep_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == {"og_sweep_limit", "og_sweep_host", "og_sweep_create", "og_sweep_destroy", "og_sweep_sync", "og_sweep_set_chunk",
                         "og_sweep_reset", "og_sweep_get_state", "og_sweep_counts_u8_dev", "og_sweep_counts_u8", "og_sweep_plan"}
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        args = _lib.SWEEP_PROTOTYPES[name][1]
        assert list(getattr(l, name).argtypes or []) == args, name
        assert len(args) == (0 if decl[name] == ["void"] else len(decl[name])), name
    assert set(decl) == set(_lib.SWEEP_PROTOTYPES)
    older = (set(_lib.PROTOTYPES) | set(_lib.CROP_PROTOTYPES) | set(_lib.CLASSIC_PROTOTYPES) | set(_lib.GATED_PROTOTYPES)
             | set(_lib.TILED_PROTOTYPES) | set(_lib.OVERLAY_PROTOTYPES))
    assert not (set(_lib.SWEEP_PROTOTYPES) & older)
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "openglottal_hip.h"' in text and '#include "openglottal_hip_gated.h"' in text      # og_track_state is the fourth header's


def test_limits():
    l = lib()
    assert l.og_sweep_limit(0) == 4194304 and l.og_sweep_limit(1) == 32 and l.og_sweep_limit(2) == 32 and l.og_sweep_limit(3) == 4096
    assert l.og_sweep_limit(4) == -1 and l.og_sweep_limit(-1) == -1


def _buffers():
    raw = np.zeros(16384, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 8
    thr = np.array([0.25, 0.5], np.float64)
    hold = np.array([0, 3, 2147483647], np.int32)
    return raw, dict(pred=base, gt=base + 512, best=base + 1024, resets=base + 2048, fc=base + 4096, counts=base + 6144, boxes=base + 8192), thr, hold


def _call(fn, h, b, thr_arr, hold_arr, **kw):
    a = dict(pred=b["pred"], gt=b["gt"], best=b["best"], resets=b["resets"], N=2, H=4, W=4, thr=thr_arr.ctypes.data, n_conf=2, hold=hold_arr.ctypes.data,
             n_hold=3, max_shift=30.0, padding=8, inclusive=0, fc=b["fc"], counts=b["counts"], boxes=b["boxes"])
    a.update(kw)
    args = [a["pred"], a["gt"], a["best"], a["resets"], a["N"], a["H"], a["W"], a["thr"], a["n_conf"], a["hold"], a["n_hold"], a["max_shift"],
            a["padding"], a["inclusive"]]
    if fn.__name__ == "og_sweep_host":
        return fn(*args, None, a["fc"], a["counts"], a["boxes"])
    return fn(h, *args, a["fc"], a["counts"], a["boxes"])


def test_the_entries_refuse_bad_arguments_without_a_device():
    """Argument checks come before the first HIP call, so they can be held here; nothing touches a buffer."""
    l = lib()
    h = l.og_sweep_create()
    assert h
    try:
        raw, b, thr, hold = _buffers()
        limit = l.og_sweep_limit(0)
        for fn in (l.og_sweep_counts_u8_dev, l.og_sweep_counts_u8, l.og_sweep_host):
            if fn is not l.og_sweep_host:
                assert _call(fn, None, b, thr, hold) == OG_EINVAL
                assert b"null handle" in l.og_last_error()
            for k in ("n_conf", "n_hold"):
                for v in (0, 33, -1):
                    assert _call(fn, h, b, thr, hold, **{k: v}) == OG_EINVAL
                    assert k.encode() in l.og_last_error()
            assert _call(fn, h, b, thr, hold, H=1, W=limit + 1) == OG_EINVAL
            assert str(limit).encode() in l.og_last_error()
            assert _call(fn, h, b, thr, hold, H=2048, W=2049) == OG_EINVAL
            for off in (1, 2, 4):
                assert _call(fn, h, b, thr, hold, thr=thr.ctypes.data + off) == OG_EINVAL
                assert b"conf_thres must be aligned to 8" in l.og_last_error()
            for name in ("counts", "fc", "boxes", "best", "hold"):
                for off in (1, 2, 3):
                    assert _call(fn, h, b, thr, hold, **{name: (hold.ctypes.data if name == "hold" else b[name]) + off}) == OG_EINVAL
                    assert b"must be aligned to 4" in l.og_last_error()
            for v in (-1, 2, 7):
                assert _call(fn, h, b, thr, hold, inclusive=v) == OG_EINVAL
                assert b"inclusive" in l.og_last_error()
            assert _call(fn, h, b, thr, hold, N=-1) == OG_EINVAL
            assert _call(fn, h, b, thr, hold, H=0) == OG_EINVAL
            assert _call(fn, h, b, thr, hold, max_shift=-1.0) == OG_EINVAL
            assert _call(fn, h, b, thr, hold, max_shift=float("nan")) == OG_EINVAL
            assert _call(fn, h, b, thr, hold, thr=None) == OG_EINVAL and _call(fn, h, b, thr, hold, hold=None) == OG_EINVAL
            bad_hold = np.array([0, -1, 3], np.int32)
            assert _call(fn, h, b, thr, hold, hold=bad_hold.ctypes.data) == OG_EINVAL
            assert b"max_hold[1]" in l.og_last_error()
            assert _call(fn, h, b, thr, hold, N=0) == 0                           # N = 0: nothing to do
            for name in ("pred", "gt", "best", "fc", "counts"):                   # required buffers
                assert _call(fn, h, b, thr, hold, **{name: None}) == OG_EINVAL
        st = gated.TrackState()
        assert l.og_sweep_get_state(h, 0, C.addressof(st)) == OG_EINVAL          # no call yet: no grid, no configuration
        assert l.og_sweep_get_state(None, 0, C.addressof(st)) == OG_EINVAL and l.og_sweep_get_state(h, 0, None) == OG_EINVAL
        assert l.og_sweep_set_chunk(h, -1) == OG_EINVAL and l.og_sweep_set_chunk(h, 4097) == OG_EINVAL
        assert l.og_sweep_set_chunk(h, 7) == 0 and l.og_sweep_set_chunk(h, 0) == 0
        assert l.og_sweep_set_chunk(None, 4) == OG_EINVAL and l.og_sweep_sync(None) == OG_EINVAL and l.og_sweep_reset(None) == OG_EINVAL
        assert l.og_sweep_sync(h) == 0 and l.og_sweep_reset(h) == 0              # no stream yet: nothing to wait for, nothing to clear
        assert not raw.any()                                                      # nothing touched a device or a buffer
    finally:
        l.og_sweep_destroy(h)
    l.og_sweep_destroy(None)


def test_the_sweep_sources_hold_no_inline_assembly():
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_sweep.inc")).read()
    assert "asm" not in src
    for k in ("k_sweep_sat_rows", "k_sweep_sat_cols", "k_sweep_track", "k_sweep_lookup"):
        assert f"void {k}(" in src, k
    assert '#include "og_sweep.inc"' in open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_api.hip")).read()
