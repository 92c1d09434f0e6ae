"""The guard-zone harness (tests/buffer_guard.py) judged on planted faults, the host-only entry points held to their declared
extents, and the completeness rule: every function of include/openglottal_hip.h that takes a caller's buffer is either in the
extents matrix or exempt for a stated reason.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import buffer_guard as G
from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1000


# ── the harness on fake entries written in numpy ────────────────────────────────
def _fake(fault=None):
    """out[i] = src[i] + 1 over N bytes, with one planted fault."""
    def call(p):
        src, out = G.view(p["src"] - 8, N + 16), G.view(p["out"] - 8, N + 16)   # (8 bytes of the neighbourhood on each side)
        res = src[8:8 + N] + np.uint8(1)
        if fault == "unwritten":
            out[8:8 + 417] = res[:417]
            out[8 + 418:8 + N] = res[418:]
            return 0
        if fault == "reads-slack":
            res = res.copy()
            res[N - 1] = src[8 + N]          # the first byte past the input's payload
        out[8:8 + N] = res
        if fault == "before":
            out[7] = 0
        if fault == "after":
            out[8 + N] = 0
        if fault == "writes-input":
            src[8 + 5] ^= 0xFF
        return 0
    return call


def _run(fault):
    src = np.random.RandomState(0).randint(0, 200, N).astype(np.uint8)
    return G.run_guarded("fake", f"fault={fault}", _fake(fault), {"src": src}, {"out": N})


def test_a_clean_entry_passes_and_the_layout_is_as_stated():
    out = _run(None)
    assert np.array_equal(out["out"], np.random.RandomState(0).randint(0, 200, N).astype(np.uint8) + np.uint8(1))
    r = G.Region("x", 100, "host", G.guard_bytes(100), G.GUARD_FILL)
    assert r.ptr % 256 == 0 and r.lo >= 64 << 10 and r.snapshot().size - r.hi >= 64 << 10 and np.all(r.snapshot() == 0xA5)
    assert G.guard_bytes(1 << 20) == 1 << 20


@pytest.mark.parametrize("fault,want", [
    ("before", ("guard-before", "out", -1, -1, 1)),
    ("after", ("guard-after", "out", 0, 0, 1)),
    ("unwritten", ("unwritten", "out", 417, 417, 1)),
    ("reads-slack", ("slack-dependent", "out", N - 1, N - 1, 1)),
    ("writes-input", ("input-modified", "src", 5, 5, 1)),
])
def test_every_planted_fault_is_reported_at_its_offset(fault, want):
    with pytest.raises(G.BufferFault) as e:
        _run(fault)
    assert [f.key() for f in e.value.faults] == [want], e.value
    msg = str(e.value)   # names the entry, the case, the buffer, the guard, the offsets and the count
    assert "fake" in msg and f"fault={fault}" in msg and want[1] in msg and want[0] in msg and f"{want[2]:+d}" in msg and "1 byte" in msg


# ── host-only entries ──────────────────────────────────────────────────────────
def test_bgr2gray_host_extents():
    rs = np.random.RandomState(1)
    for n in (1, 255, 3 * 45 * 77):
        bgr = rs.randint(0, 256, (n, 3), dtype=np.uint8)
        out = G.run_guarded("og_bgr2gray_host", f"n={n}", lambda p: lib().og_bgr2gray_host(p["bgr"], n, p["gray"]),
                            {"bgr": bgr}, {"gray": n})
        b, g, r = (bgr[:, i].astype(np.int64) for i in range(3))
        assert np.array_equal(out["gray"], ((b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15).astype(np.uint8))


def test_linear_taps_host_extents():
    from openglottal_amd.geometry import _linear_taps

    for src_len, dst_len in ((45, 32), (1, 300), (300, 1), (77, 48), (64, 131)):
        out = G.run_guarded("og_linear_taps_host", f"{src_len}->{dst_len}",
                            lambda p: lib().og_linear_taps_host(src_len, dst_len, p["i0"], p["i1"], p["frac"], p["a1"]),
                            {}, {k: 4 * dst_len for k in ("i0", "i1", "frac", "a1")})
        i0, i1, frac = _linear_taps(dst_len, src_len)[:3]
        assert np.array_equal(out["i0"].view(np.int32), i0) and np.array_equal(out["i1"].view(np.int32), i1)
        assert np.array_equal(out["frac"].view(np.float32), np.asarray(frac, np.float32))


def _geometry(H, W, imgsz):
    names = ("net_h", "net_w", "new_h", "new_w", "pad_top", "pad_left")

    def call(p):
        return lib().og_yolo_letterbox_geometry(H, W, imgsz, *[C.cast(p[k], C.POINTER(C.c_int)) for k in names],
                                                C.cast(p["gain"], C.POINTER(C.c_double)))
    out = G.run_guarded("og_yolo_letterbox_geometry", f"{H}x{W}->{imgsz}", call, {}, dict({k: 4 for k in names}, gain=8))
    return [int(out[k].view(np.int32)[0]) for k in names], float(out["gain"].view(np.float64)[0])


def test_yolo_letterbox_geometry_and_host_extents():
    from openglottal_amd.yolo import letterbox_bgr

    rs = np.random.RandomState(2)
    for (H, W), ch in (((33, 70), 3), ((100, 120), 1), ((299, 500), 3), ((224, 256), 1), ((1, 300), 3)):
        (nh, nw, ch_, cw, top, left), gain = _geometry(H, W, 256)
        assert nh % 32 == 0 and nw % 32 == 0 and gain == min(256 / H, 256 / W) and 0 <= top < 32 and 0 <= left < 32
        src = rs.randint(0, 256, (H, W, ch), dtype=np.uint8)
        out = G.run_guarded("og_yolo_letterbox_host", f"{H}x{W}x{ch}",
                            lambda p: lib().og_yolo_letterbox_host(p["src"], H, W, ch, 256, p["out"]), {"src": src}, {"out": nh * nw * 3})
        want = letterbox_bgr(np.repeat(src, 3, axis=2) if ch == 1 else src, 256)[0]
        assert np.array_equal(out["out"].reshape(nh, nw, 3), want) and ch_ > 0 and cw > 0


def test_misaligned_pointers_are_refused_by_the_host_only_entries():
    """The header's rule: a buffer of int32 / float elements is 4-byte aligned, of double / int64 8-byte aligned; u8 buffers
    need nothing.  A pointer that violates it is OG_EINVAL before anything is written."""
    buf = G.Region("b", 4096, "host", G.guard_bytes(4096), G.GUARD_FILL)
    a = buf.ptr
    for k in range(4):
        args = [a, a + 1024, a + 2048, a + 3072]
        for off in (1, 2):
            bad = list(args)
            bad[k] += off
            assert lib().og_linear_taps_host(10, 20, *bad) == -1, (k, off)
    ints = [a + 16 * i for i in range(6)]
    for k in range(6):
        bad = list(ints)
        bad[k] += 2
        assert lib().og_yolo_letterbox_geometry(100, 120, 256, *[C.cast(v, C.POINTER(C.c_int)) for v in bad],
                                                C.cast(a + 128, C.POINTER(C.c_double))) == -1, k
    assert lib().og_yolo_letterbox_geometry(100, 120, 256, *[C.cast(v, C.POINTER(C.c_int)) for v in ints],
                                            C.cast(a + 132, C.POINTER(C.c_double))) == -1
    assert np.all(buf.snapshot() == G.GUARD_FILL)      # nothing was written by any refused call
    assert lib().og_bgr2gray_host(a + 1, 100, a + 2049) == 0      # u8 buffers: any address


# ── completeness ─────────────────────────────────────────────────────────────
# Functions with a pointer parameter (other than the handle and `const char*` names) that the matrix does NOT cover, and why.
EXEMPT = {
    "og_free": "takes back a pointer of og_malloc; no extent",
    "og_memcpy_h2d": "plumbing: hipMemcpy of the byte count the caller states",
    "og_memcpy_d2h": "plumbing: hipMemcpy of the byte count the caller states",
    "og_unet_create": "reads n_levels ints on the host; nothing is written",
    "og_unet_set_tensor": "copies a host tensor whose shape the caller states; checked by the parity tests' loads",
    "og_yolo_set_tensor": "copies a host tensor whose shape the caller states; checked by the parity tests' loads",
    "og_timer_stop": "one host float, written by the host after the event wait",
    "og_unet_profile": "profile recorder: host arrays bounded by max_entries (tests/test_gpu_bench_config.py)",
    "og_unet_clock_probe": "diagnostic recorder bounded by max_entries; not on the product path",
    "og_unet_clock_probe_raw": "diagnostic: a fixed 4 x 1024 table; not on the product path",
    "og_unet_plan": "plan recorder: host text bounded by cap (tests/test_launch_plan.py)",
    "og_unet_plan_resized": "plan recorder: host text bounded by cap (tests/test_resize_host.py)",
    "og_yolo_plan": "plan recorder: host text bounded by cap (tests/test_yolo_layer_ref_f32.py)",
    "og_yolo_last_launches": "diagnostic recorder: host text bounded by cap (tests/test_yolo_layer_ref_f32.py); not on the product path",
}
HOST_ONLY = {"og_bgr2gray_host", "og_linear_taps_host", "og_yolo_letterbox_host", "og_yolo_letterbox_geometry"}   # above


def _functions_with_caller_buffers():
    text = open(os.path.join(ROOT, "include", "openglottal_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for m in re.finditer(r"\b(og_\w+)\s*\(([^()]*)\)\s*;", text):
        name, params = m.group(1), [p.strip() for p in m.group(2).split(",")]
        bufs = [p for p in params if "*" in p and not re.match(r"(og_unet|og_yolo)\s*\*\s*h$", p) and not re.match(r"const\s+char\s*\*", p)]
        if bufs:
            out[name] = bufs
    return out


def test_every_entry_point_with_a_caller_buffer_is_in_the_matrix_or_exempt():
    import test_gpu_buffer_extents as M

    fns = _functions_with_caller_buffers()
    assert len(fns) > 30 and "og_unet_segment_u8_dev" in fns and "og_yolo_detect_u8_end" in fns and "og_unet_sync" not in fns
    assert not (set(M.MATRIX) & set(EXEMPT)) and not (HOST_ONLY & set(EXEMPT))
    for name in fns:
        assert name in M.MATRIX or name in HOST_ONLY or name in EXEMPT, f"{name}{fns[name]}: not covered by the extents matrix and not exempt"
    for name in list(M.MATRIX) + list(EXEMPT) + list(HOST_ONLY):
        assert name in fns, f"{name}: listed, but the header has no such function with a caller's buffer"
    for name, test in M.MATRIX.items():
        assert all(callable(getattr(M, t, None)) for t in test.split()), (name, test)
