"""-m gpu: the device-touching entry points of include/openglottal_hip_gate.h held to the buffer extents their callers declare
(tests/buffer_guard.py): guards untouched, every declared byte written, results independent of the slack around the inputs, inputs
unchanged, payloads bit-identical to the same call on plain buffers -- at a frame size that is not the network's and whose rows are
no multiple of 16 bytes, for one frame and for 70 frames in three micro-batches.  The host twin is held the same way in
tests/test_gate_host.py."""
import ctypes as C

import numpy as np
import pytest

import buffer_guard as G
import gate_cases as GC
from openglottal_amd import gated, synth
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

# entry point -> the test of this module that puts it inside guards (tests/test_gate_abi.py checks this table against the header)
GATE_MATRIX = {
    "og_gate_select_dev": "test_select",
    "og_gate_gather_dev": "test_gather_and_scatter",
    "og_gate_scatter_dev": "test_gather_and_scatter",
    "og_gated_segment_kept_dev": "test_resident_frames",
    "og_gated_stream_kept_u8": "test_host_streaming",
    "og_gated_stream_kept_frames_u8": "test_host_streaming",
}

H, W = 99, 101
THR = 0.5
_E = {}


def engine():
    if "e" not in _E:
        import openglottal_amd as og
        from openglottal_amd.yolo import YoloV8Detector

        feats = (4, 8, 16, 32)
        m = og.UNet(1, 1, feats)
        m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=0.0))
        m.to("cuda:0").eval()
        _E["e"] = gated.GatedEngine(m, YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0"))
    return _E["e"]


def frames(B, ch):
    rs = np.random.RandomState(79 + ch)
    return rs.randint(0, 256, (B, H, W, 3) if ch == 3 else (B, H, W), dtype=np.uint8)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


def test_select():
    e = engine()
    for B in (1, 70, 513):
        boxes = GC.boxes_for(GC.patterns(B)["all" if B == 1 else "random"], W, H)
        want = GC.keep_of(boxes)
        n = len(want)
        assert n >= 1
        # keep is declared as the n entries the call writes: one more would show as a dirty guard
        out = G.run_guarded("og_gate_select_dev", f"B={B}", lambda p: lib().og_gate_select_dev(e._h, p["boxes"], B, p["keep"], p["count"]),
                            {"boxes": boxes}, {"keep": 4 * n, "count": 4}, "device", e.sync)
        assert out["count"].view(np.int32)[0] == n and np.array_equal(out["keep"].view(np.int32), want)


def test_gather_and_scatter():
    e = engine()
    B = 70
    rs = np.random.RandomState(3)
    keep = GC.keep_of(GC.boxes_for(GC.patterns(B)["random"], W, H))
    n = len(keep)
    assert 0 < n < B
    for row_bytes in (4, 16, H * W, H * W * 3):
        rows = rs.randint(1, 256, (B, row_bytes), dtype=np.uint8)
        out = G.run_guarded("og_gate_gather_dev", f"row_bytes={row_bytes}",
                            lambda p: lib().og_gate_gather_dev(e._h, p["src"], row_bytes, p["keep"], n, p["dst"]),
                            {"src": rows, "keep": keep}, {"dst": n * row_bytes}, "device", e.sync)
        assert same(out["dst"], rows[keep])
        want = np.zeros((B, row_bytes), np.uint8)
        want[keep] = rows[:n]
        out = G.run_guarded("og_gate_scatter_dev", f"row_bytes={row_bytes}",
                            lambda p: lib().og_gate_scatter_dev(e._h, p["src"], row_bytes, p["keep"], n, B, p["dst"]),
                            {"src": rows[:n], "keep": keep}, {"dst": B * row_bytes}, "device", e.sync)
        assert same(out["dst"], want)


def test_resident_frames():
    e = engine()
    for ch in (3, 1):
        for B in (1, 70):
            fr = frames(B, ch)
            for regime in ("alternating", "all", "none"):
                boxes = GC.boxes_for(GC.patterns(B)[regime], W, H)
                for with_mask in (True, False):
                    kept = C.c_int32(-1)
                    out = G.run_guarded("og_gated_segment_kept_dev", f"ch={ch} B={B} {regime} mask={with_mask}",
                                        lambda p: lib().og_gated_segment_kept_dev(e._h, p["src"], B, H, W, ch, 256, 256, THR, p["boxes"], p["mask"],
                                                                                  p["area"], C.addressof(kept)),
                                        {"src": fr, "boxes": boxes}, {"area": 4 * B, "mask": B * H * W if with_mask else None}, "device", e.sync)
                    assert kept.value == len(GC.keep_of(boxes))
                    _, want = e.model.segment_resized(fr, net=256, threshold=THR, boxes=boxes, want_mask=False)
                    assert same(out["area"], want.astype(np.int32))


def test_host_streaming():
    e = engine()
    try:
        for ch in (3, 1):
            for B in (1, 70):
                fr = frames(B, ch)
                resets = np.zeros(B, np.uint8)
                resets[B // 2] = 1
                e.set_option("stage_kib", max(1, 25 * H * W * ch // 1024))
                conf = float(np.median(e.yolo.detect_frames(fr, 0.0)[:, 4])) if B > 1 else 0.0
                e.reset()
                want = e.run(fr, conf=conf, threshold=THR, resets=resets, want_best=True, want_mask=True, skip_unboxed=True)
                args = (B, H, W, ch, 256, 256, 256, conf, THR)
                for outs in (("area", "boxes", "best", "mask"), ("area",), ("area", "mask")):
                    sizes = {"area": 4 * B, "boxes": 16 * B if "boxes" in outs else None, "best": 20 * B if "best" in outs else None,
                             "mask": B * H * W if "mask" in outs else None, "kept": 4}
                    label = f"ch={ch} B={B} outs={'+'.join(outs)}"

                    def whole(p):
                        check(lib().og_gated_reset(e._h))
                        return lib().og_gated_stream_kept_u8(e._h, p["frames"], *args, p["resets"], p["area"], p["boxes"], p["best"], p["mask"], p["kept"])
                    out = G.run_guarded("og_gated_stream_kept_u8", label, whole, {"frames": fr, "resets": resets}, sizes)
                    assert all(same(out[k], want[k]) for k in outs) and out["kept"].view(np.int32)[0] == want["kept"], label

                    def by_pointers(p):
                        check(lib().og_gated_reset(e._h))
                        fb = H * W * ch
                        ptrs = (C.c_void_p * B)(*[p["frames"] + i * fb for i in range(B)])
                        return lib().og_gated_stream_kept_frames_u8(e._h, ptrs, *args, p["resets"], p["area"], p["boxes"], p["best"], p["mask"],
                                                                    p["kept"])
                    out = G.run_guarded("og_gated_stream_kept_frames_u8", label, by_pointers, {"frames": fr, "resets": resets}, sizes)
                    assert all(same(out[k], want[k]) for k in outs) and out["kept"].view(np.int32)[0] == want["kept"], label
    finally:
        e.set_option("stage_kib", 65536)
    print(G.report())
