"""-m gpu: the device-touching entry points of include/openglottal_hip_classic.h held to the buffer extents their callers declare
(tests/buffer_guard.py): guards untouched, every declared byte written, results independent of the slack around the inputs,
inputs unchanged, payloads bit-identical to the same call on plain buffers -- and equal to the host composition.  A box outside the
frame and an empty box are among the inputs."""
import ctypes as C

import numpy as np
import pytest

import buffer_guard as G
import classic_cases as K
from openglottal_amd import classic as CL
from openglottal_amd._lib import check, lib
from openglottal_amd.utils import normalize_box

pytestmark = pytest.mark.gpu

OG_EINVAL = -1

# entry point -> the test of this module that puts it inside guards (tests/test_classic_abi.py checks this table against the header)
CLASSIC_MATRIX = {
    "og_vft_guided_init_u8": "test_init",
    "og_vft_guided_stream_u8": "test_host_streaming",
    "og_vft_guided_stream_frames_u8": "test_host_streaming",
    "og_vft_guided_u8_dev": "test_resident_frames",
    "og_otsu_in_box_u8": "test_otsu",
    "og_otsu_in_box_u8_dev": "test_otsu",
    "og_vft_guided_get_state": "test_init",
}

H, W, B = 32, 48, 11
SEED = 61.5


def inputs(ch):
    frames, boxes = K.sequence(44, B, H, W)
    boxes[2] = (60, 40, 90, 70)          # outside the frame
    boxes[3] = (12, 9, 12, 20)           # empty
    boxes[4] = None
    src = frames if ch == 3 else np.ascontiguousarray(frames[..., 1])
    return src, boxes, np.array([normalize_box(b, W, H) for b in boxes], np.int32)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


def test_init():
    e = CL.Classic()
    for ch in (1, 3):
        src, boxes, bx = inputs(ch)
        for which, box in (("first", bx[0].copy()), ("empty", bx[3].copy()), ("none", None)):
            def call(p):
                rc = lib().og_vft_guided_init_u8(e._h, p["frames"], 2, H, W, ch, p["box4"], p["thresh"])
                return rc or lib().og_vft_guided_get_state(e._h, p["state"])
            out = G.run_guarded("og_vft_guided_init_u8", f"ch={ch} box={which}", call, {"frames": src[:2], "box4": box}, {"thresh": 8, "state": 8})
            roi = boxes[0] if which == "first" else (0, 0, W, H)
            want = CL.percentile_host(CL.box_hist_host(src[1], roi), 30)
            assert out["thresh"].view(np.float64)[0] == want == out["state"].view(np.float64)[0]


def test_host_streaming():
    e = CL.Classic()
    for ch, chunk in ((1, 4), (3, 32)):
        src, boxes, bx = inputs(ch)
        e.set_chunk(chunk)
        want = CL.guided_vft_host(src, boxes, SEED)
        wanted = {"mask": np.stack(want[0]), "area": want[1], "thresh": want[2]}
        for outs in (("mask", "area", "thresh"), ("area",), ("area", "mask")):
            sizes = {"mask": B * H * W if "mask" in outs else None, "area": 4 * B, "thresh": 8 * B if "thresh" in outs else None}
            label = f"ch={ch} chunk={chunk} outs={'+'.join(outs)}"

            def whole(p):
                check(lib().og_vft_guided_set_state(e._h, SEED))
                return lib().og_vft_guided_stream_u8(e._h, p["frames"], B, H, W, ch, p["boxes"], p["mask"], p["area"], p["thresh"])
            out = G.run_guarded("og_vft_guided_stream_u8", label, whole, {"frames": src, "boxes": bx}, sizes)
            assert all(same(out[k], wanted[k]) for k in outs), label

            def by_pointers(p):
                check(lib().og_vft_guided_set_state(e._h, SEED))
                fb = H * W * ch
                ptrs = (C.c_void_p * B)(*[p["frames"] + i * fb for i in range(B)])
                return lib().og_vft_guided_stream_frames_u8(e._h, ptrs, B, H, W, ch, p["boxes"], p["mask"], p["area"], p["thresh"])
            out = G.run_guarded("og_vft_guided_stream_frames_u8", label, by_pointers, {"frames": src, "boxes": bx}, sizes)
            assert all(same(out[k], wanted[k]) for k in outs), label


def test_resident_frames():
    e = CL.Classic()
    sync = lambda: check(lib().og_classic_sync(e._h), "og_classic_sync")
    for ch, chunk in ((3, 4), (1, 32)):
        src, boxes, bx = inputs(ch)
        e.set_chunk(chunk)
        want = CL.guided_vft_host(src, boxes, SEED)
        wanted = {"mask": np.stack(want[0]), "area": want[1], "thresh": want[2]}
        for outs in (("mask", "area", "thresh"), ("area",)):
            sizes = {"mask": B * H * W if "mask" in outs else None, "area": 4 * B, "thresh": 8 * B if "thresh" in outs else None}

            def call(p):
                check(lib().og_vft_guided_set_state(e._h, SEED))
                return lib().og_vft_guided_u8_dev(e._h, p["frames"], B, H, W, ch, p["boxes"], p["mask"], p["area"], p["thresh"])
            out = G.run_guarded("og_vft_guided_u8_dev", f"ch={ch} chunk={chunk} outs={'+'.join(outs)}", call, {"frames": src, "boxes": bx},
                                sizes, "device", sync)
            assert all(same(out[k], wanted[k]) for k in outs)


def test_otsu():
    e = CL.Classic(chunk=4)
    sync = lambda: check(lib().og_classic_sync(e._h), "og_classic_sync")
    for ch in (1, 3):
        src, boxes, bx = inputs(ch)
        for want_mask in (True, False):
            sizes = {"mask": B * H * W if want_mask else None, "area": 4 * B, "T": 4 * B}
            host = G.run_guarded("og_otsu_in_box_u8", f"ch={ch} mask={want_mask}",
                                 lambda p: lib().og_otsu_in_box_u8(e._h, p["frames"], B, H, W, ch, p["boxes"], p["mask"], p["area"], p["T"]),
                                 {"frames": src, "boxes": bx}, sizes)
            dev = G.run_guarded("og_otsu_in_box_u8_dev", f"ch={ch} mask={want_mask}",
                                lambda p: lib().og_otsu_in_box_u8_dev(e._h, p["frames"], B, H, W, ch, p["boxes"], p["mask"], p["area"], p["T"]),
                                {"frames": src, "boxes": bx}, sizes, "device", sync)
            assert all(same(host[k], dev[k]) for k in host)
            area = host["area"].view(np.int32)
            assert area[0] > 0 and not area[[2, 3, 4]].any()
            for i in (0, 1, 9):
                assert host["T"].view(np.int32)[i] == CL.otsu_threshold_host(CL.box_hist_host(src[i], boxes[i]))


def test_misaligned_pointers_are_refused_with_all_guards_intact():
    e = CL.Classic()
    e.thresh = SEED
    src, boxes, bx = inputs(1)
    for bad, offs in (("boxes", (1, 2)), ("area", (1, 2)), ("thresh", (1, 4))):
        for off in offs:
            def call(p):
                q = dict(p)
                q[bad] += off
                return lib().og_vft_guided_stream_u8(e._h, q["frames"], B, H, W, 1, q["boxes"], q["mask"], q["area"], q["thresh"])
            rc, pay, faults = G.guarded_call(call, {"frames": src, "boxes": bx}, {"mask": B * H * W, "area": 4 * B + 8, "thresh": 8 * B + 8})
            assert rc == OG_EINVAL and not faults and all((v == G.GUARD_FILL).all() for v in pay.values()), (bad, off, faults)
    assert e.thresh == SEED                                  # a refused call does not move the threshold
    _, area = e.guided_vft(src, boxes, want_mask=False)      # and the handle stays usable
    assert np.array_equal(area, CL.guided_vft_host(src, boxes, SEED)[1])
    print(G.report())
