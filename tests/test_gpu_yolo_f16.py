"""GPU (-m gpu): the detector's opt-in f16 mode (``YoloV8Detector(..., precision="f16")``, og_yolo option ``"precision"`` 2).

(a) every named tensor of the chain against the float64 per-launch reference (tests/yolo_f16_ref.py) at kappa 16, from the GPU's
    own input taps, at 256 x 256 and 96 x 160, B = 1 / 2 / 192, with the stacked head chain and without;
(b) ``pred`` against the float64 decode of the GPU's own f32 logits (the f32 path's ``decode_tolerance``), ``best`` = its arg-max;
(c) per-frame, submit / result, ``detect_frames``, ``detect_batch`` at B = 1 / 3 / 192 and the device entry point: equal bits;
(d) end to end against the f32 oracle within twice the CPU emulation's own measured error (E_BOX, E_CONF below; re-measured by
    tests/test_yolo_f16_ref.py), same top-1 anchor wherever the oracle separates its top two confidences by more than 2 E_CONF;
(e) TemporalDetector and the gated area waveform over the f16 backend; precision 2 -> 0 -> 2 on one handle; OG_ERANGE.
"""
import numpy as np
import pytest

import yolo_f16_ref as R
import openglottal_amd as og
from openglottal_amd import synth
from openglottal_amd._lib import OpenGlottalHipError
from openglottal_amd.yolo import YoloV8Detector
from oracle import yolo_layer_ref as YR
from oracle import yolo_oracle as Y

pytestmark = pytest.mark.gpu

# (d): the emulation's measured error against the f32 oracle ``Y.candidates`` on e2e_frames(), the larger of NCHW and
# channels_last (tests/test_yolo_f16_ref.py::test_end_to_end_margins_and_oracle_separation re-measures both and asserts
# E / 2 <= measured <= E)
E2E_WEIGHTS = dict(seed=7, cls_bias=1.0)
E_BOX = 1.1e-3     # px; measured 1.00e-3 (NCHW), 1.09e-3 (channels_last)
E_CONF = 4.5e-5    # measured 4.40e-5 (NCHW), 3.60e-5 (channels_last); the oracle separates 14 of the 16 frames


def e2e_frames(n=16):
    return np.stack([synth.bench_frame_bgr(i) for i in range(n)])


def frames(n, h=256, w=256, seed=5):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3), dtype=np.uint8)


def decode_tolerance(H, W):   # as tests/test_gpu_yolo_layer_parity.py
    return 16 * float(np.spacing(np.float32(max(H, W)))), 8 * 2.0 ** -24


@pytest.fixture(scope="module")
def det():
    sd = synth.make_yolov8_state_dict(seed=7)
    return sd, YoloV8Detector(sd, device="cuda:0", precision="f16")


@pytest.mark.parametrize("head_fused", [1, 0])
@pytest.mark.parametrize("B", [1, 2, 192])
@pytest.mark.parametrize("shape", [(256, 256), (96, 160)])
def test_every_launch_against_float64_at_kappa_16_and_decode(det, shape, B, head_fused):
    sd, d = det
    H, W = shape
    idx = sorted({0, 1, B // 2, B - 1} & set(range(B)))   # judged frames: the first two, the middle and the last of the launch
    nread = len(idx)
    fr = frames(B, H, W, seed=H + W + B)
    d.set_option("head_fused", head_fused)
    try:
        best, pred = d.detect_batch(fr, conf=0.25, want_pred=True)
        taps = {n: d.activation(n, B, cap=B * 4 * H * W)[idx] for n in R.tap_names(sd)}   # (model.0 is the largest: 4 H W per frame)
    finally:
        d.set_option("head_fused", 1)
    taps["input"] = Y.preprocess_bgr(fr[idx]).numpy()
    dw = R.device_weights(sd)
    need, first_fail = {}, None
    for spec in R.launches(sd):
        try:
            need[spec["name"]] = R.check_launch(spec, dw, taps, idx)
        except AssertionError as ex:   # keep going: the table below shows every launch, the first failure is raised after it
            need[spec["name"]] = float("nan")
            first_fail = first_fail or ex
    print(f"f16 detector B={B} {H}x{W} head_fused={head_fused}: needed kappa per launch (of {R.KAPPA_F16:g}) "
          + " ".join(f"{k}={v:.2f}" for k, v in need.items()))
    if first_fail:
        raise first_fail
    # (b) decode of the GPU's own f32 logits
    ref = YR.decode([taps[f"model.22.cv2.{l}.2"] for l in range(3)], [taps[f"model.22.cv3.{l}.2"] for l in range(3)], H, W)
    tb, tc = decode_tolerance(H, W)
    eb = float(np.abs(pred[idx, :, :4] - ref[..., :4]).max())
    ec = float(np.abs(pred[idx, :, 4] - ref[..., 4]).max())
    print(f"decode max|dbox| {eb:.3g} px (tol {tb:.3g}) max|dconf| {ec:.3g} (tol {tc:.3g})")
    assert eb <= tb and ec <= tc, (eb, ec)
    for l in range(3):   # the existing names keep their meaning
        assert np.array_equal(d.activation(f"box{l}", 1), taps[f"model.22.cv2.{l}.2"][:1])
        assert np.array_equal(d.activation(f"cls{l}", 1), taps[f"model.22.cv3.{l}.2"][:1])
    assert np.array_equal(d.activation("model.2", 1), taps["model.2.cv2"][:1])
    for b in range(B):
        i = int(np.argmax(pred[b, :, 4]))
        assert np.array_equal(best[b], pred[b, i]) if pred[b, i, 4] > 0.25 else best[b, 4] == -1


def test_new_tap_names_are_served_in_f32_mode_too():
    sd = synth.make_yolov8_state_dict(seed=7)
    d = YoloV8Detector(sd, device="cuda:0")
    fr = frames(2, seed=3)
    d.detect_batch(fr)
    with_torch = Y.forward(sd, Y.preprocess_bgr(fr))[1]
    for n in R.tap_names(sd):
        assert np.all(np.isfinite(d.activation(n, 2))), n
    got = d.activation("model.4.cv2", 2)
    assert np.array_equal(got, d.activation("model.4", 2))
    assert np.abs(got - with_torch["model.4"].numpy()).max() <= 2e-4 * max(1.0, float(with_torch["model.4"].abs().max()))
    cv1 = d.activation("model.9.cv1", 2)
    import torch
    import torch.nn.functional as F
    assert np.array_equal(d.activation("model.9.m.1", 2), F.max_pool2d(torch.from_numpy(cv1), 5, 1, 2).numpy())


def _row(xy, cf):
    return np.concatenate([xy[0], cf]).astype(np.float32) if len(cf) else np.array([0, 0, 0, 0, -1], np.float32)


@pytest.mark.parametrize("shape,n", [((256, 256), 256), ((160, 256), 192)])
def test_every_call_shape_returns_the_same_bits(det, shape, n):
    import torch
    _, d = det
    H, W = shape
    fr = np.stack([synth.bench_frame_bgr(i) for i in range(n)]) if shape == (256, 256) else frames(n, H, W, seed=17)
    whole = d.detect_frames(fr, 0.25)
    per_frame = np.stack([_row(*d(f, 0.25)) for f in fr])
    np.testing.assert_array_equal(per_frame, whole)
    halves = []
    for f in fr:
        d.submit(f, 0.25)
        halves.append(_row(*d.result()))
    np.testing.assert_array_equal(np.stack(halves), whole)
    raw = d.detect_batch(fr, 0.25)
    for nb in (1, 3, 192):
        parts = np.concatenate([d.detect_batch(fr[i:i + nb], 0.25) for i in range(0, n, nb)])
        np.testing.assert_array_equal(parts, raw)
    np.testing.assert_array_equal(d.detect_dev(torch.from_numpy(fr).cuda(), n, H, W, 0.25), raw)
    hit = raw[:, 4] >= 0
    np.testing.assert_array_equal(whole[hit], raw[hit])
    assert hit.any()


def test_end_to_end_against_the_f32_oracle_within_the_emulations_margin():
    sd = synth.make_yolov8_state_dict(**E2E_WEIGHTS)
    d = YoloV8Detector(sd, device="cuda:0", precision="f16")
    fr = e2e_frames()
    _, pred = d.detect_batch(fr, 0.25, want_pred=True)
    ref = Y.candidates(sd, fr).astype(np.float64)
    eb = float(np.abs(pred[..., :4] - ref[..., :4]).max())
    ec = float(np.abs(pred[..., 4] - ref[..., 4]).max())
    print(f"f16 detector against the f32 oracle: max|dbox| {eb:.4g} px (2 E_BOX {2 * E_BOX:.4g}) max|dconf| {ec:.4g} (2 E_CONF {2 * E_CONF:.4g})")
    assert eb <= 2 * E_BOX and ec <= 2 * E_CONF, (eb, ec)
    top2 = np.sort(ref[..., 4], axis=1)[:, -2:]
    apart = (top2[:, 1] - top2[:, 0]) > 2 * E_CONF
    assert apart.sum() * 2 >= len(fr)
    assert np.array_equal(np.argmax(pred[apart, :, 4], 1), np.argmax(ref[apart, :, 4], 1))


def test_temporal_detector_and_gated_waveform_over_the_f16_backend(det):
    _, d = det
    td = og.TemporalDetector(d, conf=0.25)
    fr = frames(6, seed=11)
    raw = d.detect_batch(fr, 0.25)
    outs = [td.detect(f) for f in fr]
    td2 = og.TemporalDetector(lambda f, c: (np.zeros((0, 4), np.float32), np.zeros(0, np.float32)))
    exp = [td2.update(None, None, 256, 256) if b[4] < 0 else td2.update(b[None, :4], b[4:5], 256, 256) for b in raw]
    assert outs == exp
    assert any(o is not None for o in outs)
    feats = (32, 64, 128, 256)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5))
    m.to("cuda:0").eval()
    from openglottal_amd.features import area_waveform
    from openglottal_amd.utils import bgr_to_gray
    fr = frames(5, seed=21)
    wave = area_waveform(list(fr), og.TemporalDetector(d), m)
    masks, _, _ = m.segment(np.stack([bgr_to_gray(f) for f in fr]))
    td = og.TemporalDetector(d)
    for i, f in enumerate(fr):
        b = td.detect(f)
        want = 0.0 if b is None else float(np.sum(masks[i][b[1]:b[3], b[0]:b[2]] > 0))
        assert wave[i] == want


def test_switching_precision_on_one_handle_matches_fresh_handles():
    sd = synth.make_yolov8_state_dict(seed=7)
    fr = frames(5, seed=33)
    f32 = YoloV8Detector(sd, device="cuda:0").detect_batch(fr, 0.25, want_pred=True)
    f16 = YoloV8Detector(sd, device="cuda:0", precision="f16").detect_batch(fr, 0.25, want_pred=True)
    assert not np.array_equal(f32[1], f16[1])
    d = YoloV8Detector(sd, device="cuda:0", precision="f16")
    for prec, want in ((2, f16), (0, f32), (2, f16), (0, f32)):
        d.set_option("precision", prec)
        got = d.detect_batch(fr, 0.25, want_pred=True)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        np.testing.assert_array_equal(d.detect_batch(fr[:1], 0.25)[0], want[0][0])   # the one-frame path of the same handle
    for v in (1, 3):
        with pytest.raises(OpenGlottalHipError):
            d.set_option("precision", v)


def test_overflowing_weights_raise_erange_and_the_handle_stays_usable():
    sd = synth.make_yolov8_state_dict(seed=7)
    big = dict(sd)
    big["model.3.bn.weight"] = sd["model.3.bn.weight"] * np.float32(1e6)   # model.3's activations ~1e5..1e6: beyond f16
    fr = frames(3, seed=41)
    d = YoloV8Detector(big, device="cuda:0", precision="f16")
    with pytest.raises(OpenGlottalHipError, match="f16 range"):
        d.detect_batch(fr, 0.25)
    with pytest.raises(OpenGlottalHipError, match="f16 range"):
        d(fr[0], 0.25)
    d.set_option("precision", 0)
    want = YoloV8Detector(big, device="cuda:0").detect_batch(fr, 0.25)
    np.testing.assert_array_equal(d.detect_batch(fr, 0.25), want)
    ok = YoloV8Detector(sd, device="cuda:0", precision="f16")   # and a sane weight set raises nothing
    ok.detect_batch(fr, 0.25)
