"""-m gpu: the gated engine (`og_gated_stream_u8`) against the staged gated pass as it stood before the engine --
`features._detect_block` (the detector's batched call, then `TemporalDetector.update` frame by frame on the host) and
`features.area_waveform(engine="staged")` / the U-Net's streamed entries with those boxes.  The staged pass is the yardstick;
`area`, `boxes`, `best` and `mask` must be equal bit for bit, and so must the Python detector's state afterwards.

The detector's confidence threshold of a case is the median of the detector's own raw confidences on the case's frames, so that
about half of the frames have a detection: the staged boxes must then hold a fresh box, a held box and a `None`, which each case
asserts on the STAGED output before it compares anything."""
import numpy as np
import pytest

import openglottal_amd as og
from openglottal_amd import features, gated, synth
from openglottal_amd.yolo import YoloV8Detector

pytestmark = pytest.mark.gpu

N = 70
FEATS = (4, 8, 16, 32)
CASES = {                       # name -> (H, W, channels, precision)
    "bgr-256x256": (256, 256, 3, "f32"),        # the letterbox is the identity, the U-Net runs its plain chain
    "bgr-96x160": (96, 160, 3, "f32"),
    "gray-100x120": (100, 120, 1, "f32"),
    "bgr-96x160-f16": (96, 160, 3, "f16"),      # both networks at "precision" 2
}
_NETS, _REF = {}, {}


def nets(precision):
    if precision not in _NETS:
        m = og.UNet(1, 1, FEATS)
        m.load_state_dict(synth.make_unet_state_dict(FEATS, seed=5, head_scale=3.0, head_bias=0.0))
        m.to("cuda:0").eval()
        if precision == "f16":
            m.set_option("precision", 2)
        d = YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0", precision=precision)
        _NETS[precision] = (m, d, gated.GatedEngine(m, d))
    return _NETS[precision]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def det_state(det):
    return (det._centre, det._size, det._misses)


def reference(name):
    """The staged pass over the case's frames, computed once: frames, conf, best, boxes, area, mask, the detector's final state."""
    if name in _REF:
        return _REF[name]
    H, W, ch, precision = CASES[name]
    m, d, _ = nets(precision)
    rs = np.random.RandomState(H * 1000 + W + ch)
    fr = rs.randint(0, 256, (N, H, W, 3) if ch == 3 else (N, H, W), dtype=np.uint8)
    raw = d.detect_frames(fr, 0.0)[:, 4]                       # the top candidate of every frame, whatever its confidence
    conf = float(np.median(raw))
    best = d.detect_frames(fr, conf)
    det = og.TemporalDetector(d, conf=conf)
    boxes = features._detect_block(fr, det)
    # which kinds of frames the staged boxes hold, by the Python state machine's own bookkeeping
    td, kinds = og.TemporalDetector(d, conf=conf), []
    for i in range(N):
        b = td.update(best[i:i + 1, :4], best[i:i + 1, 4], W, H) if best[i, 4] >= 0 else td.update(None, None, W, H)
        kinds.append("none" if b is None else ("fresh" if td._misses == 0 else "held"))
    print(name, "conf", conf, {k: kinds.count(k) for k in ("fresh", "held", "none")})
    assert all(kinds.count(k) >= 1 for k in ("fresh", "held", "none")), kinds
    assert [k == "none" for k in kinds] == [bool(b[0] < 0) for b in boxes]
    det2 = og.TemporalDetector(d, conf=conf)
    area = features.area_waveform(fr, det2, m, engine="staged")
    if (H, W) == (256, 256):
        mask, area2 = m.segment_stream(fr, boxes=boxes, want_mask=True)
    else:
        mask, area2 = m.segment_resized(fr, net=256, boxes=boxes, want_mask=True)
    assert np.array_equal(area, area2.astype(np.float64)) and det_state(det) == det_state(det2)
    assert area.max() > 0 and (mask > 0).any()
    _REF[name] = dict(fr=fr, conf=conf, best=best, boxes=boxes, area=area2, mask=mask, state=det_state(det2), H=H, W=W, ch=ch)
    return _REF[name]


def stage_for(e, r, frames_per_micro_batch=25):
    kib = max(1, frames_per_micro_batch * r["H"] * r["W"] * r["ch"] // 1024)
    mbs, _ = gated.plan(N, r["H"], r["W"], r["ch"], kib)
    assert len(mbs) >= 3 and mbs[-1][1] < mbs[0][1], mbs       # at least three micro-batches, the last one partial
    e.set_option("stage_kib", kib)
    return mbs


@pytest.mark.parametrize("as_list", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_the_engine_equals_the_staged_pass_bit_for_bit(name, as_list):
    r = reference(name)
    m, d, e = nets(CASES[name][3])
    try:
        stage_for(e, r)
        e.set_params()
        e.reset()
        out = e.run(list(r["fr"]) if as_list else r["fr"], conf=r["conf"], want_boxes=True, want_best=True, want_mask=True)
    finally:
        e.set_option("stage_kib", 65536)
    assert same_bits(out["best"], r["best"]), np.flatnonzero((out["best"] != r["best"]).any(1))[:5]
    assert same_bits(out["boxes"], r["boxes"]), np.flatnonzero((out["boxes"] != r["boxes"]).any(1))[:5]
    assert same_bits(out["area"], r["area"]), np.flatnonzero(out["area"] != r["area"])[:5]
    assert same_bits(out["mask"], r["mask"])
    st = e.get_state()
    want = r["state"]
    assert st.as_tuple() == ((0.0, 0.0, 0, 0, 0, 0) if want[0] is None else (float(want[0][0]), float(want[0][1]), want[1][0], want[1][1], want[2], 1))
    # areas alone (no optional output), at the default setting (one micro-batch)
    e.reset()
    assert same_bits(e.run(r["fr"], conf=r["conf"], want_boxes=False)["area"], r["area"])


def test_a_second_call_continues_the_state_and_reset_restarts_it():
    r = reference("bgr-96x160")
    m, d, e = nets("f32")
    e.set_params()
    e.reset()
    a = e.run(r["fr"][:41], conf=r["conf"])
    b = e.run(r["fr"][41:], conf=r["conf"])
    assert same_bits(np.concatenate([a["boxes"], b["boxes"]]), r["boxes"]) and same_bits(np.concatenate([a["area"], b["area"]]), r["area"])
    # without a reset the tracker goes on from frame 69's state: that is the host twin started from the same state
    st = e.get_state()
    c = e.run(r["fr"][:20], conf=r["conf"])
    want = gated.track_host(st, gated.params_of(), r["best"][:20], r["W"], r["H"])
    assert same_bits(c["boxes"], want) and e.get_state().as_tuple() == st.as_tuple()
    e.reset()
    assert same_bits(e.run(r["fr"][:20], conf=r["conf"])["boxes"], r["boxes"][:20])
    # resets inside a call: every frame on its own (eval_bagls.py:164-166) is the host twin with the same resets
    e.reset()
    every = e.run(r["fr"], conf=r["conf"], resets=np.ones(N, np.uint8))
    st0 = gated.TrackState()
    assert same_bits(every["boxes"], gated.track_host(st0, gated.params_of(), r["best"], r["W"], r["H"], np.ones(N, np.uint8)))
    assert (every["boxes"][r["best"][:, 4] >= 0, 0] >= 0).all() and (every["boxes"][r["best"][:, 4] < 0, 0] < 0).all()


@pytest.mark.parametrize("name", ["bgr-96x160", "gray-100x120", "bgr-96x160-f16"])
def test_area_waveform_auto_equals_staged_and_leaves_the_detector_as_staged_does(name):
    r = reference(name)
    m, d, _ = nets(CASES[name][3])
    for src in (r["fr"], list(r["fr"])):
        det = og.TemporalDetector(d, conf=r["conf"])
        n0 = gated.GatedEngine.passes
        wave = features.area_waveform(src, det, m)             # engine="auto" is the default
        assert gated.GatedEngine.passes == n0 + 1              # ... and it took the device engine
        assert wave.dtype == np.float64 and np.array_equal(wave, r["area"].astype(np.float64))
        got, want = det_state(det), r["state"]
        assert got == want and (want[0] is None or all(type(v) is np.float32 for v in got[0])) and type(got[2]) is int
        assert det.crop_size == (None if want[1] is None else tuple(want[1]))
        # a following detect() goes on from that state exactly as after the staged pass
        ds = og.TemporalDetector(d, conf=r["conf"])
        ds._centre, ds._size, ds._misses = want
        assert det.detect(r["fr"][0]) == ds.detect(r["fr"][0])


def test_what_auto_leaves_to_the_staged_pass():
    r = reference("bgr-96x160")
    m, d, _ = nets("f32")
    ref = r["area"].astype(np.float64)
    n0 = gated.GatedEngine.passes
    assert np.array_equal(features.area_waveform(r["fr"], og.TemporalDetector(d, conf=r["conf"]), m, engine="staged"), ref)
    d.detect_frames = d.detect_frames                           # overridden on the instance (tests/test_gpu_yolo_resized.py::test_g5 does that)
    try:
        assert np.array_equal(features.area_waveform(r["fr"], og.TemporalDetector(d, conf=r["conf"]), m), ref)
    finally:
        del d.detect_frames

    m.segment_resized = m.segment_resized                       # ... or an entry of the staged pass on the model (tests/test_gpu_dist.py records its route so)
    try:
        assert np.array_equal(features.area_waveform(r["fr"], og.TemporalDetector(d, conf=r["conf"]), m), ref)
    finally:
        del m.segment_resized

    class Mine(og.TemporalDetector):                            # not a plain TemporalDetector
        pass
    assert np.array_equal(features.area_waveform(r["fr"], Mine(d, conf=r["conf"]), m), ref)
    mixed = list(r["fr"][:30]) + [np.ascontiguousarray(f[:64, :96]) for f in r["fr"][30:40]]     # two shapes
    w_mixed = features.area_waveform(mixed, og.TemporalDetector(d, conf=r["conf"]), m)
    assert np.array_equal(w_mixed, features.area_waveform(mixed, og.TemporalDetector(d, conf=r["conf"]), m, engine="staged"))
    assert gated.GatedEngine.passes == n0                       # none of them ran the device engine
    sq = reference("bgr-256x256")                               # frames at network size: measured level or behind, left to the staged pass
    assert np.array_equal(features.area_waveform(sq["fr"], og.TemporalDetector(d, conf=sq["conf"]), m), sq["area"].astype(np.float64))
    assert gated.GatedEngine.passes == n0
    det = og.TemporalDetector(d, conf=sq["conf"])               # ... unless the engine is asked for by name
    assert np.array_equal(features.area_waveform(sq["fr"], det, m, engine="device"), sq["area"].astype(np.float64))
    assert gated.GatedEngine.passes == n0 + 1 and det_state(det) == sq["state"]
    with pytest.raises(og.OpenGlottalHipError):
        features.area_waveform(mixed, og.TemporalDetector(d, conf=r["conf"]), m, engine="device")
    with pytest.raises(ValueError):
        features.area_waveform(r["fr"], og.TemporalDetector(d, conf=r["conf"]), m, engine="both")
