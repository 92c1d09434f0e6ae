"""GPU: the detector on frames of any size, letterboxed on the device.

The specification is the host composition ``YoloV8Detector.detect_frames_host``: ``letterbox_bgr`` per frame in numpy, the network at
network size, the f32 scale-back.  The device path (``k_letterbox_bgr`` -> the unchanged network -> ``og_scale_box``) must return
the same five floats per frame BIT FOR BIT: the letterboxed u8 image is the same, so the network sees the same input, and the
scale-back is the same f32 expression.  Frames are RandomState noise: any wrong tap, coefficient or pad changes bytes.
"""
import ctypes as C

import numpy as np
import pytest

import openglottal_amd as og
from openglottal_amd import synth
from openglottal_amd._lib import lib
from openglottal_amd.yolo import YoloV8Detector, letterbox_bgr

pytestmark = pytest.mark.gpu

OG_EINVAL = -1
SHAPES = [(480, 640), (640, 480), (360, 640), (299, 500), (500, 299), (100, 120), (128, 128), (256, 512), (33, 700), (250, 250),
          (224, 256), (256, 256)]
G2_SHAPES = [(480, 640), (299, 500), (500, 299), (100, 120), (33, 700), (256, 512)]
CONF = 0.25


@pytest.fixture(scope="module")
def dets():
    sd = synth.make_yolov8_state_dict(seed=7)
    return {"f32": YoloV8Detector(sd, device="cuda:0"), "f16": YoloV8Detector(sd, device="cuda:0", precision="f16")}


def frames(n, h, w, ch=3, seed=None):
    rs = np.random.RandomState(h * 1000 + w + ch if seed is None else seed)
    return rs.randint(0, 256, (n, h, w, 3) if ch == 3 else (n, h, w), dtype=np.uint8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_g1_device_letterbox_equals_letterbox_bgr_byte_for_byte(dets, shape, ch):
    fr = frames(3, *shape, ch=ch)
    got = dets["f32"].letterbox_dev(fr)
    for i in range(3):
        f = fr[i] if ch == 3 else np.repeat(fr[i][..., None], 3, axis=-1)
        ref = letterbox_bgr(f, 256)[0]
        assert got[i].shape == ref.shape and np.array_equal(got[i], ref), (shape, ch, i)


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("shape", G2_SHAPES)
def test_g2_detect_frames_equals_the_host_composition_bit_for_bit(dets, shape, precision):
    d = dets[precision]
    fr = frames(70, *shape)
    n0 = d.launch_count("k_letterbox_bgr")
    try:
        for lb in (0, 1):                       # 1: one-frame calls take the latency kernels -- on both sides
            d.set_option("latency_batch", lb)
            for B in (1, 3, 70):
                ref = d.detect_frames_host(fr[:B], CONF)
                got = d.detect_frames(fr[:B], CONF)
                print(f"{shape} {precision} latency_batch={lb} B={B}: hits {int((ref[:, 4] >= 0).sum())}")
                assert got.dtype == np.float32 and same_bits(got, ref), (shape, precision, lb, B, got[:3], ref[:3])
    finally:
        d.set_option("latency_batch", 1)
    assert d.launch_count("k_letterbox_bgr") > n0    # ... and it did run on the device


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_g2_the_shapes_are_covered_by_detections(dets, precision):
    """A shape without a hit in any frame compares only `no detection` rows: at least 5 of the 6 shapes must have one, on both
    sides (the 33x700 noise case, 12 content rows between two pads, is allowed to have none)."""
    d = dets[precision]
    for fn in (d.detect_frames_host, d.detect_frames):
        hit = {s: bool((fn(frames(3, *s), CONF)[:, 4] >= 0).any()) for s in G2_SHAPES}   # (the first frames of G2's 70)
        print(precision, fn.__name__, hit)
        assert sum(hit.values()) >= 5, hit


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_g3_every_one_frame_entry_returns_the_same_bits(dets, precision):
    import torch

    d = dets[precision]
    f = frames(1, 360, 640)[0]
    ref = d.detect_frames(f[None], CONF)[0]
    assert same_bits(ref, d.detect_frames_host(f[None], CONF)[0])
    assert ref[4] >= 0                                   # (a detection: the comparison below is about coordinates)
    xy, cf = d(f, CONF)
    assert same_bits(xy[0], ref[:4]) and same_bits(cf, ref[4:5])
    d.submit(f, CONF)
    xy, cf = d.result()
    assert same_bits(xy[0], ref[:4]) and same_bits(cf, ref[4:5])
    got = d.detect_resized_dev(torch.from_numpy(f).to("cuda:0"), 1, 360, 640, 3, CONF)   # boxes scaled by k_scale_boxes
    assert same_bits(got[0], ref)
    g = frames(1, 360, 640, ch=1)[0]                     # gray: one byte per pixel up, replicated on the device
    ref1 = d.detect_frames_host(g[None], CONF)[0]
    assert same_bits(d.detect_frames(g[None], CONF)[0], ref1)
    assert same_bits(d.detect_resized_dev(torch.from_numpy(g).to("cuda:0"), 1, 360, 640, 1, CONF)[0], ref1)


def test_g4_chunked_staging_changes_no_bit(dets):
    d = dets["f32"]
    fr = frames(7, 360, 640)
    ref = d.detect_frames(fr, CONF)
    assert same_bits(ref, d.detect_frames_host(fr, CONF))
    try:
        n0 = d.launch_count("k_letterbox_bgr")
        d.set_option("source_stage_kib", 2 * 360 * 640 * 3 // 1024)      # room for two frames: four uploads
        assert same_bits(d.detect_frames(fr, CONF), ref)
        assert d.launch_count("k_letterbox_bgr") - n0 == 4
        d.set_option("source_stage_kib", 100)                            # less than one frame: each frame is staged alone
        assert same_bits(d.detect_frames(fr, CONF), ref)
        assert d.launch_count("k_letterbox_bgr") - n0 == 4 + 7
    finally:
        d.set_option("source_stage_kib", 65536)


def test_g5_gated_area_waveform_equals_the_host_letterbox(dets):
    from openglottal_amd import features

    d = dets["f32"]
    feats = (4, 8, 16, 32)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-0.4))
    m.to("cuda:0").eval()
    fr = frames(40, 480, 640)
    boxes = features._detect_block(list(fr), og.TemporalDetector(d))
    wave = features.area_waveform(list(fr), og.TemporalDetector(d), m)
    d.detect_frames = d.detect_frames_host               # the baseline: letterbox on the host
    try:
        boxes_h = features._detect_block(list(fr), og.TemporalDetector(d))
        wave_h = features.area_waveform(list(fr), og.TemporalDetector(d), m)
    finally:
        del d.detect_frames
    assert boxes.dtype == np.int32 and np.array_equal(boxes, boxes_h) and (boxes[:, 0] >= 0).any()
    assert np.array_equal(wave.astype(np.int64), wave_h.astype(np.int64)) and np.array_equal(wave, wave_h) and wave.max() > 0


def test_g6_begin_while_a_call_is_in_flight_is_refused(dets):
    d = dets["f32"]
    f = frames(1, 360, 640)[0]
    ref = d.detect_frames_host(f[None], CONF)[0]
    p = f.ctypes.data
    assert lib().og_yolo_detect_resized_u8_begin(d._h, p, 1, 360, 640, 3, 256, CONF) == 0
    try:
        assert lib().og_yolo_detect_resized_u8_begin(d._h, p, 1, 360, 640, 3, 256, CONF) == OG_EINVAL
        best = np.empty((1, 5), np.float32)
        assert lib().og_yolo_detect_resized_u8(d._h, p, 1, 360, 640, 3, 256, CONF, best.ctypes.data) == OG_EINVAL
    finally:
        out = np.empty((1, 5), np.float32)
        assert lib().og_yolo_detect_u8_end(d._h, out.ctypes.data) == 0
    assert same_bits(out[0], ref)                        # the call in flight was not disturbed
    assert same_bits(d.detect_frames(f[None], CONF)[0], ref)   # and the next plain call succeeds and matches


@pytest.mark.parametrize("shape", [(256, 256), (224, 256)])
def test_g7_identity_shapes_take_the_plain_path(dets, shape):
    d = dets["f32"]
    fr = frames(3, *shape)
    n0, s0 = d.launch_count("k_letterbox_bgr"), d.launch_count("k_scale_boxes")
    got = d.detect_frames(fr, CONF)
    one = d(fr[0], CONF)
    d.submit(fr[0], CONF)
    two = d.result()
    assert (d.launch_count("k_letterbox_bgr"), d.launch_count("k_scale_boxes")) == (n0, s0)
    raw = d.detect_batch(fr, CONF).copy()
    raw[raw[:, 4] < 0, :4] = 0                           # (`no detection` rows carry zero coordinates)
    assert (raw[:, 4] >= 0).any() and same_bits(got, raw)
    one_raw = d.detect_batch(fr[:1], CONF)[0]
    for xy, cf in (one, two):
        assert len(cf) == (one_raw[4] >= 0)
        if len(cf):
            assert same_bits(xy[0], one_raw[:4]) and same_bits(cf, one_raw[4:5])
