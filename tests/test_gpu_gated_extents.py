"""-m gpu: the device-touching entry points of include/openglottal_hip_gated.h held to the buffer extents their callers declare
(tests/buffer_guard.py): guards untouched, every declared byte written, results independent of the slack around the inputs, inputs
unchanged, payloads bit-identical to the same call on plain buffers -- at a frame size that is not the network's, for one frame
and for 70 frames in three micro-batches.  Then the error paths: each returns its code with payloads and guards untouched, and a
good call afterwards gives the same bits as before."""
import ctypes as C

import numpy as np
import pytest

import buffer_guard as G
import track_cases as T
from openglottal_amd import gated, synth
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

OG_EINVAL = -1

# entry point -> the test of this module that puts it inside guards (tests/test_gated_abi.py checks this table against the header)
GATED_MATRIX = {
    "og_gated_stream_u8": "test_host_streaming",
    "og_gated_stream_frames_u8": "test_host_streaming",
    "og_track_boxes_dev": "test_resident_rows",
    "og_gated_set_params": "test_state_and_parameters",
    "og_gated_set_state": "test_state_and_parameters",
    "og_gated_get_state": "test_state_and_parameters",
}

H, W = 96, 160
CONF, THR = 0.25, 0.5
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
    rs = np.random.RandomState(77 + ch)
    return rs.randint(0, 256, (B, H, W, 3) if ch == 3 else (B, H, W), dtype=np.uint8)


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


def stream_args(B, ch):
    return (B, H, W, ch, 256, 256, 256, CONF, THR)


def test_host_streaming():
    e = engine()
    try:
        for ch in (3, 1):
            for B in (1, 70):
                fr = frames(B, ch)
                resets = np.zeros(B, np.uint8)
                resets[B // 2] = 1
                e.set_option("stage_kib", max(1, 25 * H * W * ch // 1024))
                e.reset()
                want = e.run(fr, conf=CONF, threshold=THR, resets=resets, want_best=True, want_mask=True)
                assert want["area"].max() > 0
                for outs in (("area", "boxes", "best", "mask"), ("area",), ("area", "mask")):
                    sizes = {"area": 4 * B, "boxes": 16 * B if "boxes" in outs else None, "best": 20 * B if "best" in outs else None,
                             "mask": B * H * W if "mask" in outs else None}
                    label = f"ch={ch} B={B} outs={'+'.join(outs)}"

                    def whole(p):
                        check(lib().og_gated_reset(e._h))
                        return lib().og_gated_stream_u8(e._h, p["frames"], *stream_args(B, ch), p["resets"], p["area"], p["boxes"], p["best"], p["mask"])
                    out = G.run_guarded("og_gated_stream_u8", label, whole, {"frames": fr, "resets": resets}, sizes)
                    assert all(same(out[k], want[k]) for k in outs), label

                    def by_pointers(p):
                        check(lib().og_gated_reset(e._h))
                        fb = H * W * ch
                        ptrs = (C.c_void_p * B)(*[p["frames"] + i * fb for i in range(B)])
                        return lib().og_gated_stream_frames_u8(e._h, ptrs, *stream_args(B, ch), p["resets"], p["area"], p["boxes"], p["best"],
                                                               p["mask"])
                    out = G.run_guarded("og_gated_stream_frames_u8", label, by_pointers, {"frames": fr, "resets": resets}, sizes)
                    assert all(same(out[k], want[k]) for k in outs), label
                out = G.run_guarded("og_gated_stream_u8", f"ch={ch} B={B} no resets",
                                    lambda p: check(lib().og_gated_reset(e._h)) or lib().og_gated_stream_u8(
                                        e._h, p["frames"], *stream_args(B, ch), None, p["area"], p["boxes"], None, None),
                                    {"frames": fr}, {"area": 4 * B, "boxes": 16 * B})
                e.reset()
                assert same(out["boxes"], e.run(fr, conf=CONF, threshold=THR)["boxes"])
    finally:
        e.set_option("stage_kib", 65536)


def test_resident_rows():
    e = engine()
    w = T.short_walk(700, 5)
    e.set_params()
    for B in (1, 70, 700):
        for with_resets in (True, False):
            def call(p):
                check(lib().og_gated_reset(e._h))
                return lib().og_track_boxes_dev(e._h, p["best"], p["resets"], B, w["W"], w["H"], p["boxes"])
            out = G.run_guarded("og_track_boxes_dev", f"B={B} resets={with_resets}", call,
                                {"best": w["best"][:B], "resets": w["resets"][:B] if with_resets else None}, {"boxes": 16 * B}, "device", e.sync)
            st = gated.TrackState()
            want = gated.track_host(st, gated.params_of(), w["best"][:B], w["W"], w["H"], w["resets"][:B] if with_resets else None)
            assert same(out["boxes"], want) and e.get_state().as_tuple() == st.as_tuple()


def test_state_and_parameters():
    e = engine()
    w = T.short_walk(700, 6, dict(max_shift_px=12.5, padding=0, max_hold_frames=0), (100, 120))
    p0 = gated.params_of(12.5, 0, 0)
    st_in = gated.TrackState(*[t(v) for t, v in zip((float, float, int, int, int, int), w["states"][299])])
    assert st_in.has_centre == 1
    import torch

    d_best = torch.from_numpy(w["best"][300:]).to("cuda:0")
    d_box = torch.empty((400, 4), dtype=torch.int32, device="cuda:0")

    def call(p):
        rc = lib().og_gated_set_params(e._h, p["params"]) or lib().og_gated_set_state(e._h, p["state_in"])
        rc = rc or lib().og_gated_get_state(e._h, p["echo"])
        rc = rc or lib().og_track_boxes_dev(e._h, d_best.data_ptr(), None, 400, w["W"], w["H"], d_box.data_ptr())
        return rc or lib().og_gated_get_state(e._h, p["state"])
    out = G.run_guarded("og_gated_get_state", "set, echo, 400 frames, get", call,
                        {"params": np.frombuffer(bytes(p0), np.uint8), "state_in": np.frombuffer(bytes(st_in), np.uint8)}, {"echo": 24, "state": 24})
    G.CASES["og_gated_set_state"] += 1
    G.CASES["og_gated_set_params"] += 1
    assert same(out["echo"], np.frombuffer(bytes(st_in), np.uint8))
    # no resets were passed: the host twin from the same state, without them
    st = gated.TrackState.from_buffer_copy(bytes(st_in))
    want = gated.track_host(st, p0, w["best"][300:], w["W"], w["H"])
    assert same(d_box.cpu().numpy(), want) and same(out["state"], np.frombuffer(bytes(st), np.uint8))
    e.set_params()
    e.reset()


def test_error_paths_leave_every_byte_alone_and_the_handles_usable():
    e = engine()
    B, ch = 70, 3
    fr = frames(B, ch)
    e.reset()
    good = e.run(fr, conf=CONF, threshold=THR, want_best=True, want_mask=True)
    state = e.get_state().as_tuple()
    sizes = {"area": 4 * B + 8, "boxes": 16 * B + 8, "best": 20 * B + 8, "mask": B * H * W}

    def attempt(label, expect, fn):
        rc, pay, faults = G.guarded_call(fn, {"frames": fr}, sizes)
        assert rc == expect and not faults and all((v == G.GUARD_FILL).all() for v in pay.values()), (label, rc, faults)
        assert e.get_state().as_tuple() == state, label              # a refused call does not move the tracker

    l = lib()
    a = stream_args(B, ch)
    attempt("B = 0", 0, lambda p: l.og_gated_stream_u8(e._h, p["frames"], 0, *a[1:], None, p["area"], p["boxes"], p["best"], p["mask"]))
    attempt("channels", OG_EINVAL, lambda p: l.og_gated_stream_u8(e._h, p["frames"], B, H, W, 2, *a[4:], None, p["area"], p["boxes"], p["best"], p["mask"]))
    attempt("imgsz", OG_EINVAL, lambda p: l.og_gated_stream_u8(e._h, p["frames"], B, H, W, ch, 250, *a[5:], None, p["area"], p["boxes"], p["best"], p["mask"]))
    attempt("net size", OG_EINVAL, lambda p: l.og_gated_stream_u8(e._h, p["frames"], B, H, W, ch, 256, 250, 256, CONF, THR, None, p["area"], p["boxes"],
                                                                    p["best"], p["mask"]))
    attempt("null frames", OG_EINVAL, lambda p: l.og_gated_stream_u8(e._h, None, *a, None, p["area"], p["boxes"], p["best"], p["mask"]))
    attempt("null area", OG_EINVAL, lambda p: l.og_gated_stream_u8(e._h, p["frames"], *a, None, None, p["boxes"], p["best"], p["mask"]))
    for bad, offs in (("area", (1, 2)), ("boxes", (1, 2)), ("best", (1, 2))):
        for off in offs:
            def call(p):
                q = dict(p)
                q[bad] += off
                return l.og_gated_stream_u8(e._h, q["frames"], *a, None, q["area"], q["boxes"], q["best"], q["mask"])
            attempt(f"{bad}+{off}", OG_EINVAL, call)
    ptrs = (C.c_void_p * B)(*([fr.ctypes.data] * (B - 1) + [0]))
    attempt("a null frame pointer", OG_EINVAL,
            lambda p: l.og_gated_stream_frames_u8(e._h, ptrs, *a, None, p["area"], p["boxes"], p["best"], p["mask"]))
    # handles that are not finalized never become an engine
    u = l.og_unet_create((C.c_int * 4)(4, 8, 16, 32), 4, 1, 1)
    try:
        assert u and not l.og_gated_create(u, e.yolo._h) and b"finalized" in l.og_last_error()
    finally:
        l.og_unet_destroy(u)
    # ... and a good call afterwards gives the same bits, on all three handles
    e.reset()
    again = e.run(fr, conf=CONF, threshold=THR, want_best=True, want_mask=True)
    assert all(same(again[k], good[k]) for k in good)
    assert same(e.yolo.detect_frames(fr, CONF), good["best"])
    assert same(e.model.segment_resized(fr, net=256, threshold=THR, boxes=good["boxes"], want_mask=False)[1], good["area"])
    print(G.report())
