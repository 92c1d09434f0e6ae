"""-m gpu: the device-touching entry points of include/openglottal_hip_overlay.h held to the buffer extents their callers declare
(tests/buffer_guard.py): guards untouched, every declared byte written, results independent of the slack around the inputs, inputs
unchanged, payloads bit-identical to the same call on plain buffers -- and equal to the host twin.  At 40 x 56 and, above the
one-workgroup limit, 300 x 260."""
import ctypes as C

import numpy as np
import pytest

import buffer_guard as G
import overlay_cases as OC
from openglottal_amd import overlay as OV
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

OG_EINVAL = -1
STYLE = {"none": 0, "contour": 1, "fill": 2}
SHAPES = ((40, 56, 5), (300, 260, 2))                                     # H, W, B

# entry point -> the test of this module that puts it inside guards
OVERLAY_MATRIX = {
    "og_overlay_u8_dev": "test_resident_frames",
    "og_overlay_stream_u8": "test_host_streaming",
    "og_overlay_stream_frames_u8": "test_host_streaming",
}


def inputs(H, W, B, ch):
    rs = np.random.RandomState(H + ch)
    frames = OC.frames_for(B, H, W, ch, seed=W)
    masks = ((rs.rand(B, H, W) < 0.58) * 255).astype(np.uint8)
    masks[0, H // 4:H // 2, W // 4:W // 2] = 255
    masks[0, H // 4 + 2:H // 2 - 2, W // 4 + 2:W // 2 - 2] = 0
    cases = OC.box_cases(H, W)
    boxes = np.array([cases[(i + 2) % len(cases)][1] for i in range(B)], np.int32)
    boxes[1] = -1
    return frames, masks, boxes


def wanted(frames, masks, boxes, style):
    return np.stack([OV.overlay_host(frames[i], None if masks is None else masks[i], OC.ABSENT if boxes is None else boxes[i], style,
                                     normalized=True) for i in range(len(frames))])


def variants(frames, masks, boxes):
    yield "fill", masks, boxes
    yield "contour", masks, None
    yield "fill", None, boxes
    yield "none", masks, boxes


@pytest.mark.parametrize("H,W,B", SHAPES)
def test_host_streaming(H, W, B):
    e = OV.Overlay(chunk=2)
    for ch in (1, 3):
        frames, masks, boxes = inputs(H, W, B, ch)
        for style, m, b in variants(frames, masks, boxes):
            label = f"{H}x{W} ch={ch} {style} masks={m is not None} boxes={b is not None}"
            want = wanted(frames, m, b, style)
            out = G.run_guarded("og_overlay_stream_u8", label,
                                lambda p: lib().og_overlay_stream_u8(e._h, p["frames"], B, H, W, ch, p["masks"], p["boxes"], STYLE[style], p["out"]),
                                {"frames": frames, "masks": m, "boxes": b}, {"out": B * H * W * 3})
            assert np.array_equal(out["out"].reshape(want.shape), want), label

            def by_pointers(p):
                fb = H * W * ch
                ptrs = (C.c_void_p * B)(*[p["frames"] + i * fb for i in range(B)])
                return lib().og_overlay_stream_frames_u8(e._h, ptrs, B, H, W, ch, p["masks"], p["boxes"], STYLE[style], p["out"])
            out = G.run_guarded("og_overlay_stream_frames_u8", label, by_pointers, {"frames": frames, "masks": m, "boxes": b},
                                {"out": B * H * W * 3})
            assert np.array_equal(out["out"].reshape(want.shape), want), label


@pytest.mark.parametrize("H,W,B", SHAPES)
def test_resident_frames(H, W, B):
    e = OV.Overlay(chunk=2)
    sync = lambda: check(lib().og_overlay_sync(e._h), "og_overlay_sync")
    for ch in (1, 3):
        frames, masks, boxes = inputs(H, W, B, ch)
        for style, m, b in variants(frames, masks, boxes):
            label = f"{H}x{W} ch={ch} {style} masks={m is not None} boxes={b is not None}"
            out = G.run_guarded("og_overlay_u8_dev", label,
                                lambda p: lib().og_overlay_u8_dev(e._h, p["frames"], B, H, W, ch, p["masks"], p["boxes"], STYLE[style], p["out"]),
                                {"frames": frames, "masks": m, "boxes": b}, {"out": B * H * W * 3}, "device", sync)
            want = wanted(frames, m, b, style)
            assert np.array_equal(out["out"].reshape(want.shape), want), label


def test_misaligned_boxes_are_refused_with_all_guards_intact():
    H, W, B = 40, 56, 5
    e = OV.Overlay()
    frames, masks, boxes = inputs(H, W, B, 1)
    for off in (1, 2, 3):
        def call(p):
            return lib().og_overlay_stream_u8(e._h, p["frames"], B, H, W, 1, p["masks"], p["boxes"] + off, 2, p["out"])
        rc, pay, faults = G.guarded_call(call, {"frames": frames, "masks": masks, "boxes": boxes}, {"out": B * H * W * 3})
        assert rc == OG_EINVAL and not faults and (pay["out"] == G.GUARD_FILL).all(), (off, faults)
    assert np.array_equal(e.annotate(frames, masks, boxes, "fill"), wanted(frames, masks, boxes, "fill"))      # the handle stays usable
    print(G.report())
