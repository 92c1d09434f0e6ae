"""-m gpu: the device-touching entry points of include/openglottal_hip_crops.h held to the buffer extents their callers declare
(tests/buffer_guard.py, as tests/test_gpu_buffer_extents.py does for the main header): guards untouched, every declared byte
written, results independent of the slack around the inputs, inputs unchanged, payloads bit-identical to the same call on plain
buffers and to the host composition of tests/crop_cases.py."""
import ctypes as C

import numpy as np
import pytest

import buffer_guard as G
import crop_cases as K
import openglottal_amd as og
from openglottal_amd import synth
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

OG_EINVAL = -1
FEATS = (4, 8, 16, 32)

# entry point -> the test(s) of this module that put it inside guards (tests/test_crops_abi.py checks this table against the header)
CROP_MATRIX = {
    "og_unet_stream_crops_u8": "test_host_streaming",
    "og_unet_stream_frames_crops_u8": "test_host_streaming",
    "og_unet_segment_crops_area_u8_dev": "test_resident_frames",
}

OUT_OF_FRAME = (50, 50, 120, 70)
ROWS = [K.USABLE[0], (-1, -1, -1, -1), K.USABLE[5], K.SLIVER, K.USABLE[9], OUT_OF_FRAME, K.USABLE[3], K.EMPTY, K.USABLE[7]]
B = len(ROWS)

_NET = []


def net():
    if not _NET:
        m = og.UNet(1, 1, FEATS)
        m.load_state_dict(synth.make_unet_state_dict(FEATS, seed=11, head_scale=3.0, head_bias=0.5))
        _NET.append(m.to("cuda:0").eval())
    return _NET[0]


def frames(ch):
    return np.random.RandomState(40 + ch).randint(0, 256, (B, K.H, K.W, 3) if ch == 3 else (B, K.H, K.W), dtype=np.uint8)


_REF = {}


def reference(m, src, ch):
    """The host composition (raw rows: the Python wrapper would clamp the out-of-frame box as slicing does), once per channel count."""
    if ch not in _REF:
        from openglottal_amd.utils import bgr_to_gray_numpy

        m.set_chunk(32)
        _REF[ch] = K.host_composition(m, list(bgr_to_gray_numpy(src) if ch == 3 else src), ROWS, K.SIZE)
    return _REF[ch]


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


def test_host_streaming():
    m = net()
    boxes = np.array(ROWS, np.int32)
    try:
        for ch, chunk, lanes in ((1, 2, 1), (3, 2, 0), (3, 32, 0), (1, 1, 3)):
            src = frames(ch)
            want_mask, want_area = reference(m, src, ch)
            m.set_chunk(chunk)
            m.set_option("lanes", lanes)
            assert want_area[0] > 0 and not want_area[[1, 3, 5, 7]].any()
            for want in (("mask", "area"), ("area",), ("mask",)):
                outs = {"mask": B * K.H * K.W if "mask" in want else None, "area": 4 * B if "area" in want else None}
                label = f"ch={ch} chunk={chunk} lanes={lanes} want={'+'.join(want)}"
                out = G.run_guarded("og_unet_stream_crops_u8", label,
                                    lambda p: lib().og_unet_stream_crops_u8(m._h, p["frames"], B, K.H, K.W, ch, p["boxes"], K.SIZE, 0.5, p["mask"],
                                                                            p["area"]),
                                    {"frames": src, "boxes": boxes}, outs)
                assert all(same(out[k], {"mask": want_mask, "area": want_area}[k]) for k in want), label

                def by_pointers(p):
                    fb = K.H * K.W * ch
                    ptrs = (C.c_void_p * B)(*[p["frames"] + i * fb for i in range(B)])
                    return lib().og_unet_stream_frames_crops_u8(m._h, ptrs, B, K.H, K.W, ch, p["boxes"], K.SIZE, 0.5, p["mask"], p["area"])
                out = G.run_guarded("og_unet_stream_frames_crops_u8", label, by_pointers, {"frames": src, "boxes": boxes}, outs)
                assert all(same(out[k], {"mask": want_mask, "area": want_area}[k]) for k in want), label
    finally:
        m.set_chunk(32)
        m.set_option("lanes", 0)


def test_resident_frames():
    """The `_dev` entry has no compaction: the out-of-frame box, the sliver, the empty box and `no detection` run the network on a
    zero tile and still give area 0 and a zero frame; both scratch buffers are fully written."""
    m = net()
    boxes = np.array(ROWS, np.int32)
    sync = lambda: check(lib().og_unet_sync(m._h), "og_unet_sync")
    try:
        for ch, chunk in ((1, 32), (3, 2)):
            src = frames(ch)
            want_mask, want_area = reference(m, src, ch)
            m.set_chunk(chunk)
            for want in (("mask", "area"), ("area",), ("mask",)):
                outs = {"tiles": B * K.SIZE * K.SIZE, "tile_masks": B * K.SIZE * K.SIZE, "mask": B * K.H * K.W if "mask" in want else None,
                        "area": 4 * B if "area" in want else None}
                label = f"ch={ch} chunk={chunk} want={'+'.join(want)} (one out-of-frame box, one sliver)"
                out = G.run_guarded("og_unet_segment_crops_area_u8_dev", label,
                                    lambda p: lib().og_unet_segment_crops_area_u8_dev(m._h, p["src"], B, K.H, K.W, ch, p["boxes"], K.SIZE, 0.5,
                                                                                      p["tiles"], p["tile_masks"], p["mask"], p["area"]),
                                    {"src": src, "boxes": boxes}, outs, "device", sync)
                assert all(same(out[k], {"mask": want_mask, "area": want_area}[k]) for k in want), label
                tiles = out["tiles"].reshape(B, -1)
                assert not tiles[[1, 3, 5, 7]].any() and tiles[0].any()
    finally:
        m.set_chunk(32)


def test_misaligned_boxes_and_area_are_refused_with_all_guards_intact():
    m = net()
    boxes = np.array(ROWS, np.int32)
    src = frames(1)
    for bad in ("boxes", "area"):
        for off in (1, 2):
            def shifted(p, fn):
                q = dict(p)
                q[bad] += off
                return fn(q)
            host = lambda q: lib().og_unet_stream_crops_u8(m._h, q["frames"], B, K.H, K.W, 1, q["boxes"], K.SIZE, 0.5, q["mask"], q["area"])
            rc, pay, faults = G.guarded_call(lambda p: shifted(p, host), {"frames": src, "boxes": boxes}, {"mask": B * K.H * K.W, "area": 4 * B + 4})
            assert rc == OG_EINVAL and not faults and all((v == G.GUARD_FILL).all() for v in pay.values()), (bad, off, faults)

            def by_pointers(q):
                ptrs = (C.c_void_p * B)(*[q["frames"] + i * K.H * K.W for i in range(B)])
                return lib().og_unet_stream_frames_crops_u8(m._h, ptrs, B, K.H, K.W, 1, q["boxes"], K.SIZE, 0.5, q["mask"], q["area"])
            rc, pay, faults = G.guarded_call(lambda p: shifted(p, by_pointers), {"frames": src, "boxes": boxes},
                                             {"mask": B * K.H * K.W, "area": 4 * B + 4})
            assert rc == OG_EINVAL and not faults and all((v == G.GUARD_FILL).all() for v in pay.values()), (bad, off, faults)
            dev = lambda q: lib().og_unet_segment_crops_area_u8_dev(m._h, q["src"], B, K.H, K.W, 1, q["boxes"], K.SIZE, 0.5, q["tiles"],
                                                                    q["tile_masks"], q["mask"], q["area"])
            rc, pay, faults = G.guarded_call(lambda p: shifted(p, dev), {"src": src, "boxes": boxes},
                                             {"tiles": B * K.SIZE * K.SIZE, "tile_masks": B * K.SIZE * K.SIZE, "mask": B * K.H * K.W,
                                              "area": 4 * B + 4}, "device", lambda: check(lib().og_unet_sync(m._h), "og_unet_sync"))
            assert rc == OG_EINVAL and not faults and all((v == G.GUARD_FILL).all() for v in pay.values()), (bad, off, faults)
    # a misaligned frame_ptrs array
    raw = (C.c_void_p * (B + 1))(*([src.ctypes.data + i * K.H * K.W for i in range(B)] + [0]))
    area = np.zeros(B, np.int32)
    assert lib().og_unet_stream_frames_crops_u8(m._h, C.addressof(raw) + 4, B, K.H, K.W, 1, boxes.ctypes.data, K.SIZE, 0.5, None,
                                                area.ctypes.data) == OG_EINVAL
    print(G.report())
