"""CPU: the detector's float64 module references (oracle/yolo_layer_ref.py) restate yolo_oracle, their propagated bounds hold for
f32 arithmetic, and the float64 decode's tolerance is reachable by an f32 decode and misses a wrong one."""
import numpy as np
import pytest

from openglottal_amd import synth
from oracle import yolo_layer_ref as YR
from oracle import yolo_oracle as Y

H, W = 64, 96


@pytest.fixture(scope="module")
def chain():
    import torch

    sd = synth.make_yolov8_state_dict(seed=7)
    fr = np.random.RandomState(3).randint(0, 256, (2, H, W, 3), dtype=np.uint8)
    x = Y.preprocess_bgr(fr)
    with torch.no_grad():
        _, taps = Y.forward(sd, x)
    return sd, x, {k: v.numpy() for k, v in taps.items()}


def test_float64_chain_bounds_the_f32_oracle(chain):
    """The f32 torch oracle, chained from the input, stays inside the float64 chain's propagated bound at every tap."""
    sd, x, taps = chain
    ref = YR.full_forward(sd, x.numpy())
    for n in YR.MODULES:
        w = YR.check_module(n, taps[n], ref[n])
        assert w <= 1.0


def test_module_from_its_own_inputs(chain):
    """Module isolation: each module from the f32 oracle's own input taps passes, and a perturbed input is caught downstream."""
    sd, x, taps = chain
    taps = dict(taps, input=x.numpy())
    for n, (ins, _) in YR.MODULES.items():
        YR.check_module(n, taps[n], YR.module(sd, n, [taps[i] for i in ins]))
    bad = taps["model.4"].copy()
    bad[1] *= 1.0 + 2.0 ** -12                      # frame 1 of model.5's input off by 2^-12 (far above f32 rounding)
    with pytest.raises(AssertionError, match=r"model.5: .* at frame 1"):
        YR.check_module("model.5", YR.module(sd, "model.5", [bad]).v.numpy().astype(np.float32), YR.module(sd, "model.5", [taps["model.4"]]))


def _decode_f32(box, cls, stride, Hf, Wf, half=0.5):
    """the kernels' decode in numpy f32 (expf, 16-bin sums, products by the stride, clip)."""
    f = np.float32
    B, _, h, w = box.shape
    lg = box.astype(f).reshape(B, 4, 16, h * w)
    e = np.exp(lg - lg.max(2, keepdims=True)).astype(f)
    d = ((e * np.arange(16, dtype=f)[None, None, :, None]).sum(2, dtype=f) / e.sum(2, dtype=f)).astype(f)
    sy, sx = np.meshgrid(np.arange(h, dtype=f) + f(half), np.arange(w, dtype=f) + f(half), indexing="ij")
    ax, ay = sx.reshape(-1), sy.reshape(-1)
    x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
    st = f(stride)
    cx, cy = (x1 + x2) * f(0.5) * st, (y1 + y2) * f(0.5) * st
    ww, hh = (x2 - x1) * st, (y2 - y1) * st
    r = np.stack([(cx - ww * f(0.5)).clip(0, Wf), (cy - hh * f(0.5)).clip(0, Hf), (cx + ww * f(0.5)).clip(0, Wf),
                  (cy + hh * f(0.5)).clip(0, Hf)], -1).astype(f)
    conf = (f(1) / (f(1) + np.exp(-cls[:, 0].astype(f).reshape(B, h * w)))).astype(f)
    return np.concatenate([r, conf[..., None]], -1)


def test_decode_tolerance_reached_by_f32_and_missed_by_a_wrong_decode(chain):
    sd, x, taps = chain
    boxes, clss = [taps[f"box{l}"] for l in range(3)], [taps[f"cls{l}"] for l in range(3)]
    ref = YR.decode(boxes, clss, H, W)
    cand = Y.candidates(sd, np.zeros((1,) + (H, W, 3), np.uint8))       # (shape only)
    assert ref.shape[1] == cand.shape[1]
    # the tolerance of tests/test_gpu_yolo_layer_parity.py
    tb, tc = 16 * float(np.spacing(np.float32(max(H, W)))), 8 * 2.0 ** -24
    for half, ok in ((0.5, True), (0.0, False)):          # anchor centre at x + 0.5 (right) / x (a dropped half-cell offset)
        got = np.concatenate([_decode_f32(b, c, W / b.shape[-1], H, W, half) for b, c in zip(boxes, clss)], 1)
        eb, ec = np.abs(got[..., :4] - ref[..., :4]).max(), np.abs(got[..., 4] - ref[..., 4]).max()
        print("f32 decode (anchor offset %.1f): max|dbox| %.3g px (tol %.3g), max|dconf| %.3g (tol %.3g)" % (half, eb, tb, ec, tc))
        assert (eb <= tb and ec <= tc) == ok
