"""-m gpu: the two figures built on the sweep (openglottal_amd/sweep.py) against the evaluations they replace.

* `hold_ablation`: for each hold, the `unet-only` and `yolo+unet` lists and `n_det` of `evaluate()` run with
  `TemporalDetector(..., max_hold_frames=hold)`, compared with `==` on floats (both go through the reference's f32 formula), over two
  patients so that resets occur.  The detector's threshold is the median of its own raw confidences on these frames, so about half of
  the frames have a detection and the hold matters.
* `conf_sweep`: the column of a threshold with the detector's own rule (`inclusive=False`) equals `evaluate_device` run AT that
  threshold -- the detector run once at 0.001 and gated afterwards is the detector run at the threshold, because `best` is the
  arg-max candidate.  Asserted at 0.25 and at the median confidence.
"""
import json
import os

import numpy as np
import pytest

import openglottal_amd as og
from openglottal_amd import evaluate as E
from openglottal_amd import sweep, synth
from openglottal_amd.geometry import letterbox
from openglottal_amd.yolo import YoloV8Detector

pytestmark = pytest.mark.gpu

N = 48


@pytest.fixture(scope="module")
def nets(golden_dir):
    g = np.load(os.path.join(golden_dir, "unet_trained_small.npz"))
    sd = {k[2:]: g[k] for k in g.files if k.startswith("W:")}
    m = og.UNet(1, 1, tuple(int(f) for f in g["features"]))
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    return m, YoloV8Detector(synth.make_yolov8_state_dict(seed=7, cls_bias=1.0), device="cuda:0")


def test_hold_ablation_equals_evaluate_per_hold(nets):
    m, yolo = nets
    frames, gts = synth.bagls_standin(N, seed=5)
    frames = [letterbox(f, 256) for f in frames]
    gts = [letterbox(g, 256) for g in gts]
    conf = float(np.float32(np.median(yolo.detect_frames(np.stack(frames), 0.0)[:, 4])))       # (an f32: the detector compares in f32)
    patients = ["a"] * 20 + ["b"] * (N - 20)
    res = sweep.hold_ablation(frames, gts, m, og.TemporalDetector(yolo, conf=conf), holds=(0, 3, None), patients=patients)
    assert list(res) == [0, 3, None]
    n_det = []
    for hold in (0, 3, None):
        det = og.TemporalDetector(yolo, conf=conf, max_hold_frames=sweep.HOLD_FOREVER if hold is None else hold)
        agg, _, _ = E.evaluate(frames, gts, m, detector=det, patients=patients)
        got = res[hold]["agg"]
        for p in ("unet-only", "yolo+unet"):
            assert got[p]["dice"] == agg[p]["dice"] and got[p]["iou"] == agg[p]["iou"], (hold, p)
            assert got[p]["n_det"] == agg[p]["n_det"] and got[p]["n_total"] == agg[p]["n_total"] == N, (hold, p)
        want = E.summarize({p: agg[p] for p in ("unet-only", "yolo+unet")})
        assert res[hold]["summary"] == want
        n_det.append(got["yolo+unet"]["n_det"])
    print("n_det per hold", n_det, "conf", conf)
    assert 0 < n_det[0] < n_det[2] <= N and n_det[0] <= n_det[1] <= n_det[2]      # the hold matters on these frames
    sweep.print_hold_table(res)


def test_a_conf_sweep_column_equals_the_evaluation_at_that_threshold(nets, tmp_path):
    m, yolo = nets
    frames, gts = synth.bagls_standin(N, seed=5)                 # mixed sizes: letterboxed to the canvas
    det = og.TemporalDetector(yolo, conf=0.25)
    lb = np.stack([letterbox(f, 256) for f in frames])
    median = float(np.float32(np.median(yolo.detect_frames(lb, 0.0)[:, 4])))                 # (an f32: the detector compares in f32)
    confs = sorted({0.001, 0.25, median})
    path = str(tmp_path / "out" / "sweep.json")
    res, aggs = sweep.conf_sweep(frames, gts, m, det, crop_model=m, confs=confs, inclusive=False, output_json=path, want_agg=True)
    n_det = [aggs[c]["yolo+unet"]["n_det"] for c in confs]
    print("n_det per threshold", dict(zip(confs, n_det)))
    assert n_det == sorted(n_det, reverse=True) and n_det[0] > n_det[-1] >= 0 and n_det[0] > 0
    for c in (0.25, median):
        agg_d, _ = E.evaluate_device(frames, gts, m, detector=og.TemporalDetector(yolo, conf=c), crop_model=m, canvas=256)
        for p in E.PIPELINES:
            assert aggs[c][p]["dice"] == agg_d[p]["dice"] and aggs[c][p]["iou"] == agg_d[p]["iou"], (c, p)
            assert aggs[c][p]["n_det"] == agg_d[p]["n_det"] and aggs[c][p]["n_total"] == agg_d[p]["n_total"] == N, (c, p)
    # the JSON of sweep_bagls_conf.py:272-291
    got = json.load(open(path))
    assert got == res and list(got) == [str(c) for c in confs]
    for key in got:
        assert set(got[key]) == set(E.PIPELINES)
        for p in E.PIPELINES:
            assert set(got[key][p]) == {"dice_mean", "iou_mean", "dice_ge_05", "det_recall", "n_det", "n_total"}
            assert got[key][p]["dice_mean"] == float(np.mean(aggs[float(key)][p]["dice"]))
    # the script's own rule (>=) at the paper's thresholds: a run without the crop row, table printed
    res2 = sweep.conf_sweep(frames, gts, m, det)
    assert list(res2) == [str(c) for c in sweep.CONF_THRESHOLDS] and set(res2["0.25"]) == {"unet-only", "yolo+unet"}
    assert res2["0.25"]["yolo+unet"]["n_det"] >= aggs[0.25]["yolo+unet"]["n_det"]
    sweep.print_conf_table(res2)
