"""GPU (-m gpu): the YOLOv8 detector module by module against float64, its decode against a float64 decode of its own logits,
and the arg-max tie rule of both decode kernels.

* Every tapped module is recomputed in float64 from the GPU's OWN input taps (oracle/yolo_layer_ref.py), with a bound propagated
  through the module's convs; on the batched default (B = 2), a batch that takes the occupancy kernels and the one-frame latency
  path (``latency_batch`` 1: split K on every small conv), at 256 x 256 and 96 x 160.  This adds to, and replaces nothing of, the
  end-to-end 2e-4 check of tests/test_gpu_yolo.py.
* ``pred`` against the float64 decode of the GPU's own ``box*`` / ``cls*`` logits: within 16 f32 ulps of the frame size (boxes)
  and 8 * 2^-24 (confidences).
* Tie rule: with ``cls_bias`` +40 every confidence rounds to 1.0f, so the best box must be anchor 0's -- the "lowest index wins"
  contract of k_yolo_decode (batched) and k_yolo_decode_mb (latency path, cross-workgroup reduce), at B = 1 and B = 3.
"""
import numpy as np
import pytest

from openglottal_amd import synth
from openglottal_amd.yolo import YoloV8Detector
from oracle import yolo_layer_ref as YR
from oracle import yolo_oracle as Y

pytestmark = pytest.mark.gpu

NAMES = list(YR.MODULES)


def frames(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3), dtype=np.uint8)


def decode_tolerance(H, W):
    return 16 * float(np.spacing(np.float32(max(H, W)))), 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def det():
    sd = synth.make_yolov8_state_dict(seed=7)
    return sd, YoloV8Detector(sd, device="cuda:0")


@pytest.mark.parametrize("path,B,nread,latency_batch", [("batched", 2, 2, 1), ("occupancy", 192, 1, 1), ("latency", 1, 1, 1)])
@pytest.mark.parametrize("shape", [(256, 256), (96, 160)])
def test_every_module_against_float64_and_decode(det, path, B, nread, latency_batch, shape):
    sd, d = det
    H, W = shape
    fr = frames(B, H, W, seed=H + W + B)
    d.set_option("latency_batch", latency_batch)
    best, pred = d.detect_batch(fr, conf=0.25, want_pred=True)
    taps = {n: d.activation(n, nread) for n in NAMES}
    taps["input"] = Y.preprocess_bgr(fr[:nread]).numpy()
    worst = {}
    for n in NAMES:
        ins, _ = YR.MODULES[n]
        worst[n] = YR.check_module(n, taps[n], YR.module(sd, n, [taps[i] for i in ins]))
    ref = YR.decode([taps[f"box{l}"] for l in range(3)], [taps[f"cls{l}"] for l in range(3)], H, W)
    tb, tc = decode_tolerance(H, W)
    eb = float(np.abs(pred[:nread, :, :4] - ref[..., :4]).max())
    ec = float(np.abs(pred[:nread, :, 4] - ref[..., 4]).max())
    print(f"{path} B={B} {H}x{W}: worst |err|/bound per module " + " ".join(f"{k}={v:.3f}" for k, v in worst.items())
          + f"; decode max|dbox| {eb:.3g} px (tol {tb:.3g}) max|dconf| {ec:.3g} (tol {tc:.3g})")
    assert eb <= tb and ec <= tc, (eb, ec)
    for b in range(nread):
        i = int(np.argmax(pred[b, :, 4]))
        assert np.array_equal(best[b], pred[b, i]) if pred[b, i, 4] > 0.25 else best[b, 4] == -1


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("latency_batch", [0, 3], ids=["k_yolo_decode", "k_yolo_decode_mb"])
def test_all_confidences_tie_and_the_lowest_anchor_wins(B, latency_batch):
    sd = synth.make_yolov8_state_dict(seed=7, cls_bias=40.0)
    d = YoloV8Detector(sd, device="cuda:0")
    d.set_option("latency_batch", latency_batch)
    fr = frames(B, 256, 256, seed=31 + B)
    best, pred = d.detect_batch(fr, conf=0.25, want_pred=True)
    assert np.all(pred[..., 4] == np.float32(1.0)), float(pred[..., 4].min())
    for b in range(B):
        assert np.array_equal(best[b], pred[b, 0]), (b, best[b], pred[b, 0], int(np.argmax(np.all(pred[b] == best[b], -1))))
