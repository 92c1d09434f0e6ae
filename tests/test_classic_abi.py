"""The rules tests/test_crops_abi.py holds the second header to, on the third, include/openglottal_hip_classic.h: every function it
declares is exported and bound (`_lib.CLASSIC_PROTOTYPES`) and vice versa; the two older headers and their tables are untouched;
every function with a caller's buffer is in the extents matrix of tests/test_gpu_classic_extents.py, host only (and then held to
its extents here) or exempt for a stated reason; misaligned pointers are refused before anything is written.  No GPU."""
import ctypes as C
import os
import re

import numpy as np

import buffer_guard as G
import classic_cases as K
from openglottal_amd import _lib
from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL, OG_ESTATE = -1, -2
HEADER = "openglottal_hip_classic.h"

EXEMPT = {
    "og_classic_plan": "plan recorder: host text bounded by cap (tests/test_classic_plan.py)",
}
HOST_ONLY = {"og_percentile_host", "og_otsu_threshold_host", "og_box_hist_host", "og_vft_step_host", "og_blobs_host"}


def _declarations(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return {m.group(1): [p.strip() for p in m.group(2).split(",")] for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_every_function_of_the_classic_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert len(decl) == 20 and "og_vft_guided_stream_u8" in decl
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        assert getattr(l, name).argtypes == _lib.CLASSIC_PROTOTYPES[name][1]
    assert set(decl) == set(_lib.CLASSIC_PROTOTYPES), set(decl) ^ set(_lib.CLASSIC_PROTOTYPES)
    assert not (set(_lib.CLASSIC_PROTOTYPES) & (set(_lib.PROTOTYPES) | set(_lib.CROP_PROTOTYPES)))
    for name, (_, args) in _lib.CLASSIC_PROTOTYPES.items():
        n = 0 if decl[name] == ["void"] else len(decl[name])
        assert len(args) == n, name
    required = {"og_classic_create", "og_classic_destroy", "og_classic_sync", "og_vft_guided_reset", "og_vft_guided_init_u8",
                "og_vft_guided_stream_u8", "og_vft_guided_u8_dev", "og_otsu_in_box_u8", "og_otsu_in_box_u8_dev", "og_percentile_host",
                "og_otsu_threshold_host", "og_blobs_host", "og_classic_plan"}
    assert required <= set(decl)


def test_the_older_headers_still_equal_their_tables_and_are_unchanged():
    assert set(_declarations("openglottal_hip.h")) == set(_lib.PROTOTYPES)
    assert set(_declarations("openglottal_hip_crops.h")) == set(_lib.CROP_PROTOTYPES)
    assert '#include "openglottal_hip.h"' in open(os.path.join(ROOT, "include", HEADER)).read()
    assert len(_lib.PROTOTYPES) == 66 and len(_lib.CROP_PROTOTYPES) == 7


def test_every_classic_entry_with_a_caller_buffer_is_in_the_matrix_host_only_or_exempt():
    import test_gpu_classic_extents as M

    fns = {}
    for name, params in _declarations(HEADER).items():
        bufs = [p for p in params if "*" in p and not re.match(r"og_classic\s*\*\s*h$", p)]
        if bufs:
            fns[name] = bufs
    assert not (set(M.CLASSIC_MATRIX) & set(EXEMPT)) and not (HOST_ONLY & set(EXEMPT)) and not (HOST_ONLY & set(M.CLASSIC_MATRIX))
    for name in fns:
        assert name in M.CLASSIC_MATRIX or name in HOST_ONLY or name in EXEMPT, f"{name}{fns[name]}: not covered and not exempt"
    for name in list(M.CLASSIC_MATRIX) + list(EXEMPT) + list(HOST_ONLY):
        assert name in fns, f"{name}: listed, but the header has no such function with a caller's buffer"
    for name, test in M.CLASSIC_MATRIX.items():
        assert all(callable(getattr(M, t, None)) for t in test.split()), (name, test)


# ── the host-only entries inside guards ──────────────────────────────────────────
def test_host_only_entries_stay_inside_their_extents():
    rs = np.random.RandomState(2)
    hist = np.bincount(rs.randint(0, 256, 999), minlength=256).astype(np.uint32)
    out = G.run_guarded("og_percentile_host", "q=30", lambda p: lib().og_percentile_host(p["hist"], 30.0, p["out"]), {"hist": hist}, {"out": 8})
    assert out["out"].view(np.float64)[0] == np.percentile(np.repeat(np.arange(256), hist), 30)
    out = G.run_guarded("og_otsu_threshold_host", "", lambda p: lib().og_otsu_threshold_host(p["hist"], p["T"]), {"hist": hist}, {"T": 4})
    assert out["T"].view(np.int32)[0] == K.otsu_numpy(hist)
    out = G.run_guarded("og_vft_step_host", "", lambda p: lib().og_vft_step_host(100.0, 0.7, p["hist"], 30.0, p["t"], p["cut"]),
                        {"hist": hist}, {"t": 8, "cut": 4})
    assert out["t"].view(np.float64)[0] == 0.7 * 100.0 + (1 - 0.7) * float(np.percentile(np.repeat(np.arange(256), hist), 30))
    frames, _ = K.sequence(3, 1, 17, 23)
    for ch, f in ((3, frames[0]), (1, np.ascontiguousarray(frames[0][..., 1]))):
        for box in ((2, 3, 20, 15), (0, 0, 23, 17), (5, 5, 5, 9), (-1, -1, -1, -1), (10, 8, 60, 40)):
            out = G.run_guarded("og_box_hist_host", f"ch={ch} box={box}",
                                lambda p: lib().og_box_hist_host(p["frame"], 17, 23, ch, p["box"], p["hist"]),
                                {"frame": f, "box": np.array(box, np.int32)}, {"hist": 1024})
            x1, y1, x2, y2 = box
            n = 0 if x1 < 0 else max(0, min(x2, 23) - x1) * max(0, min(y2, 17) - y1)
            assert out["hist"].view(np.uint32).sum() == n
    for name, m in K.named_masks()[:14]:
        for want_mask in (True, False):
            out = G.run_guarded("og_blobs_host", f"{name} mask={want_mask}",
                                lambda p: lib().og_blobs_host(p["mask"], m.shape[0], m.shape[1], 2, p["out"], p["area"]),
                                {"mask": m}, {"out": m.size if want_mask else None, "area": 4})
            assert out["area"].view(np.int32)[0] == K.scipy_blobs(m, 2)[1]


def test_misaligned_pointers_are_refused_by_the_host_only_entries():
    buf = G.Region("b", 1 << 16, "host", G.guard_bytes(1 << 16), G.GUARD_FILL)
    a = buf.ptr
    hist, out, frame, box, mask = a, a + 2048, a + 4096, a + 8192, a + 16384
    G.view(hist, 1024)[:] = np.ones(256, np.uint32).view(np.uint8)
    G.view(box, 16)[:] = np.array([0, 0, 4, 4], np.int32).view(np.uint8)
    before = buf.snapshot()
    l = lib()
    for off in (1, 2, 3):
        assert l.og_percentile_host(hist + off, 30.0, out) == OG_EINVAL
        assert l.og_otsu_threshold_host(hist + off, out) == OG_EINVAL
        assert l.og_otsu_threshold_host(hist, out + off) == OG_EINVAL
        assert l.og_box_hist_host(frame, 8, 8, 1, box + off, out) == OG_EINVAL
        assert l.og_box_hist_host(frame, 8, 8, 1, box, out + off) == OG_EINVAL
        assert l.og_vft_step_host(1.0, 0.7, hist + off, 30.0, out, out + 8) == OG_EINVAL
        assert l.og_vft_step_host(1.0, 0.7, hist, 30.0, out, out + 8 + off) == OG_EINVAL
        assert l.og_blobs_host(mask, 8, 8, 2, mask + 64, out + off) == OG_EINVAL
    for off in (1, 2, 4):
        assert l.og_percentile_host(hist, 30.0, out + off) == OG_EINVAL
        assert l.og_vft_step_host(1.0, 0.7, hist, 30.0, out + off, out + 8) == OG_EINVAL
    assert np.array_equal(buf.snapshot(), before)          # nothing was written by any refused call
    assert l.og_blobs_host(mask + 1, 8, 8, 2, mask + 67, out) == 0        # u8 buffers: any address


def test_the_handle_refuses_bad_arguments_without_a_device():
    """Argument checks come before the first HIP call, so they can be held here: alignment, shape, limits, call order."""
    l = lib()
    h = l.og_classic_create()
    assert h
    try:
        raw = np.zeros(4096, np.uint8)
        base = raw.ctypes.data + (-raw.ctypes.data) % 8
        frames, boxes, area, th = base, base + 1024, base + 2048, base + 3072
        assert l.og_vft_guided_stream_u8(h, frames, 1, 8, 8, 1, boxes + 2, None, area, None) == OG_EINVAL
        assert b"boxes must be aligned to 4" in l.og_last_error()
        assert l.og_vft_guided_stream_u8(h, frames, 1, 8, 8, 1, boxes, None, area + 1, None) == OG_EINVAL
        assert l.og_vft_guided_stream_u8(h, frames, 1, 8, 8, 1, boxes, None, area, th + 4) == OG_EINVAL
        assert l.og_vft_guided_u8_dev(h, frames, 1, 8, 8, 1, boxes + 1, None, area, None) == OG_EINVAL
        assert l.og_otsu_in_box_u8(h, frames, 1, 8, 8, 1, boxes, None, area, area + 2) == OG_EINVAL
        assert l.og_vft_guided_init_u8(h, frames, 1, 8, 8, 1, boxes + 2, None) == OG_EINVAL
        ptrs = (C.c_void_p * 2)(frames, 0)
        assert l.og_vft_guided_stream_frames_u8(h, C.addressof(ptrs) + 4, 1, 8, 8, 1, boxes, None, area, None) == OG_EINVAL
        assert l.og_vft_guided_stream_u8(h, frames, 1, 8, 8, 2, boxes, None, area, None) == OG_EINVAL           # channels
        limit = l.og_classic_limit(0)
        assert limit == 1 << 16 and l.og_classic_limit(1) == 8 and l.og_classic_limit(3) == 64 << 20 and l.og_classic_limit(9) == -1
        assert l.og_vft_guided_stream_u8(h, frames, 1, 257, 256, 1, boxes, None, area, None) == OG_EINVAL
        assert str(limit).encode() in l.og_last_error()                                                         # the limit is in the message
        assert l.og_vft_guided_stream_u8(h, frames, 1, 8, 8, 1, boxes, None, area, None) == OG_ESTATE           # no threshold yet
        assert l.og_vft_guided_get_state(h, th) == OG_ESTATE
        for beta, q, n in ((0.7, 101.0, 2), (0.7, -1.0, 2), (0.7, 30.0, 0), (0.7, 30.0, 9), (float("nan"), 30.0, 2)):
            assert l.og_vft_guided_reset(h, beta, q, n) == OG_EINVAL
        assert l.og_vft_guided_reset(h, 0.7, 30.0, 8) == 0
        assert l.og_classic_set_chunk(h, 0) == OG_EINVAL and l.og_classic_set_chunk(h, 1025) == OG_EINVAL and l.og_classic_set_chunk(h, 7) == 0
        assert l.og_vft_guided_stream_u8(h, frames, 0, 8, 8, 1, boxes, None, area, None) == OG_ESTATE
        assert l.og_otsu_in_box_u8(h, frames, 0, 8, 8, 1, boxes, None, area, area) == 0                          # B = 0: nothing to do
        assert l.og_classic_sync(h) == 0                                                                       # no stream yet: nothing to wait for
        assert not raw.any()
    finally:
        l.og_classic_destroy(h)


def test_the_new_sources_hold_no_inline_assembly():
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_classic.inc")).read()
    assert "asm" not in src.replace("assembly", "")
    kern = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_kernels.hpp")).read()
    new = kern[kern.index("The training-free family"):]
    assert "asm" not in new and "k_blobs" in new
