"""-m gpu: `k_track_boxes` (`og_track_boxes_dev`) against its host twin `og_track_host` -- the same inline rule, so boxes and state
must be equal word for word -- on scripted rows that visit every branch (tests/track_cases.py), at the batch sizes where the kernel
changes its loop (one block of 256 frames, the block's edge, several blocks), with and without resets, over several launches, and
on the reference's own traces."""
import json
import os

import numpy as np
import pytest

import track_cases as T
from openglottal_amd import gated, synth
from openglottal_amd.yolo import YoloV8Detector

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import openglottal_amd as og

    feats = (4, 8, 16, 32)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-0.4))
    m.to("cuda:0").eval()
    e = gated.GatedEngine(m, YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0"))
    yield e
    e.close()


def device_track(e, best, W, H, resets=None, cuts=None):
    """The rows through the kernel, in one launch or cut into several; -> (boxes, state words)."""
    import torch

    n = len(best)
    d_best = torch.from_numpy(np.ascontiguousarray(best)).to("cuda:0")
    d_res = None if resets is None else torch.from_numpy(np.ascontiguousarray(resets)).to("cuda:0")
    d_box = torch.full((n, 4), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    cuts = [0, n] if cuts is None else cuts
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        e.track_dev(d_best[lo:], hi - lo, W, H, d_box[lo:], None if d_res is None else d_res[lo:])
    st = e.get_state()                                        # waits for the stream
    return d_box.cpu().numpy(), st.as_tuple()


@pytest.mark.parametrize("with_resets", [False, True])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 700])
def test_the_kernel_equals_the_host_twin(eng, B, with_resets):
    for kw, shape, seed in (({}, (256, 256), 5), (dict(max_shift_px=12.5, padding=0, max_hold_frames=0), (100, 120), 6)):
        w = T.short_walk(700, seed, kw, shape)
        p = gated.params_of(*[getattr(T.TemporalDetector(T._none_backend, **kw), k) for k in ("max_shift", "padding", "max_hold_frames")])
        best, res = w["best"][:B], (w["resets"][:B] if with_resets else None)
        st = gated.TrackState()
        want = gated.track_host(st, p, best, w["W"], w["H"], res)
        eng.set_params(p.max_shift_px, p.padding, p.max_hold_frames)
        eng.reset()
        got, state = device_track(eng, best, w["W"], w["H"], res)
        assert np.array_equal(got, want), (B, with_resets, kw, np.flatnonzero((got != want).any(1))[:5])
        assert state == st.as_tuple()
        if with_resets:                                       # ... and both equal the Python state machine the walk recorded
            assert np.array_equal(got, w["boxes"][:B]) and state == tuple(w["states"][B - 1])
        assert (want[:, 0] >= 0).any() or B < 3


def test_700_frames_as_three_launches_equal_one(eng):
    w = T.short_walk(700, 5)
    eng.set_params()
    eng.reset()
    one, s1 = device_track(eng, w["best"], w["W"], w["H"], w["resets"])
    eng.reset()
    three, s3 = device_track(eng, w["best"], w["W"], w["H"], w["resets"], cuts=[0, 130, 513, 700])
    assert np.array_equal(one, three) and s1 == s3 and np.array_equal(one, w["boxes"])
    # the state set from the host is the state the next launch starts from
    st = gated.TrackState(*[t(v) for t, v in zip((float, float, int, int, int, int), w["states"][399])])
    eng.set_state(st)
    tail, s4 = device_track(eng, w["best"][400:], w["W"], w["H"], w["resets"][400:])
    assert np.array_equal(tail, w["boxes"][400:]) and s4 == s1


def test_the_golden_traces_through_the_kernel(eng, golden_dir):
    traces = json.load(open(os.path.join(golden_dir, "detector_traces.json")))
    for name, t in traces.items():
        H, W = t["shape"][:2]
        kw = dict(t["kw"])
        det = T.TemporalDetector(T._none_backend, **kw)
        eng.set_params(det.max_shift, det.padding, det.max_hold_frames)
        eng.reset()
        got, _ = device_track(eng, T.trace_rows(t["script"], kw.get("conf", 0.25)), W, H)
        want = np.array([[-1] * 4 if b is None else b for b in t["out"]], np.int32)
        assert np.array_equal(got, want), name
