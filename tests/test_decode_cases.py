"""CPU: the nets of tests/decode_cases.py do what tests/test_gpu_yolo_select.py relies on, shown on the torch-f32 emulation of the
chain (``yolo_layer_ref.emulate_f32``) alone, with room to spare; and the selection oracle and the DFL closed form are what they say."""
import numpy as np
import pytest

import decode_cases as DC
from oracle import yolo_layer_ref as YR
from oracle import yolo_oracle as Y


def f32_sigmoid(lg):
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-np.asarray(lg, np.float32)))).astype(np.float32)


def emulated(sd, fr):
    """(conf [B,A] f32, box logits per level, class logits per level) of the emulated chain."""
    taps = YR.emulate_f32(sd, Y.preprocess_bgr(fr).numpy())
    box = [taps[f"model.22.cv2.{l}.2"] for l in range(3)]
    cls = [taps[f"model.22.cv3.{l}.2"] for l in range(3)]
    return f32_sigmoid(np.concatenate([c.reshape(len(fr), -1) for c in cls], 1)), box, cls


@pytest.mark.parametrize("shape", list(DC.TIE_CASES), ids=lambda s: f"{s[0]}x{s[1]}")
def test_tie_nets_tie_partially_with_room_to_spare(shape):
    H, W = shape
    conf, _, _ = emulated(DC.tie_net_for(H, W), DC.frames(H, W))
    st = DC.tie_stats(conf, H, W)
    print(f"tie net {H}x{W} {DC.TIE_CASES[shape]}: {DC.describe(st)}")
    DC.check_tie_conditions(st, shape)
    assert min(st["per_frame"]) >= 2 * DC.MIN_TIED, st              # the margin the GPU test's own check of its pred can lose
    assert st["A"] == sum(DC.level_sizes(H, W))
    if st["A"] > 64:
        assert any(f > 0 for f in st["first"])                       # the winner is not simply anchor 0
    # random weights, for contrast: every confidence of a frame is its own -- the tie rule never runs
    plain, _, _ = emulated(DC.base_sd(), DC.frames(H, W)[:1])
    assert DC.tie_stats(plain, H, W)["per_frame"] == [1]


def test_total_tie_nets_put_the_winner_where_the_rule_says():
    H, W = 96, 160
    A0, A1, A2 = DC.level_sizes(H, W)
    fr = DC.frames(H, W, B=1)
    for biases, first, n in (((0.0, 0.0, 0.0), 0, A0 + A1 + A2), ((1.0, 0.0, 0.0), 0, A0), ((0.0, 1.0, 0.0), A0, A1),
                             ((0.0, 0.0, 1.0), A0 + A1, A2), ((0.0, 1.0, 1.0), A0, A1 + A2)):
        conf, _, _ = emulated(DC.total_tie_net(biases), fr)
        t = DC.tied(conf[0])
        print(f"total tie, level biases {biases}: {len(t)} anchors at the maximum, first {int(t[0])}")
        assert (int(t[0]), len(t)) == (first, n)
    for bias, value in ((100.0, 1.0), (-100.0, 0.0)):                # saturation: exactly 1 and exactly 0 in f32
        conf, _, _ = emulated(DC.total_tie_net((bias,) * 3), fr)
        assert np.all(conf == np.float32(value)), (bias, np.unique(conf))


def test_select_is_the_stated_rule():
    pred = np.zeros((6, 5), np.float32)
    pred[:, 0] = np.arange(6)                                        # (the box names the row)
    pred[:, 4] = [0.25, 0.75, 0.5, 0.75, 0.75, 0.25]
    c0 = np.float32(0.75)
    assert DC.select(pred, 0.5)[0] == 1                              # lowest index of the three maxima
    assert np.array_equal(DC.select(pred, c0), DC.NONE_ROW)          # strict >
    assert DC.select(pred, np.nextafter(c0, np.float32(0)))[0] == 1
    assert DC.select(pred, 0.0)[0] == 1
    assert np.array_equal(DC.select(pred, np.nextafter(np.float32(1), np.float32(2))), DC.NONE_ROW)
    pred[:, 4] = 0.0
    assert np.array_equal(DC.select(pred, 0.0), DC.NONE_ROW)         # conf 0 at conf_thres 0: nothing passes
    assert DC.select(pred, -1.0)[0] == 0
    assert np.array_equal(DC.tied(pred[:, 4]), np.arange(6))


@pytest.mark.parametrize("bins", [(0, 0, 0, 0), (15, 15, 15, 15), (0, 15, 15, 0), (15, 0, 0, 15), (7.5, 7.5, 7.5, 7.5), ("+200",) * 4,
                                  (3, 7.5, "+200", 12)], ids=str)
def test_dfl_closed_form_is_the_float64_decode_of_the_bias(bins):
    """The DFL nets' logits are their bias at every anchor; the float64 decode of that is the closed form to 1e-30 relative (the other
    bins weigh exp(-80)), and at 15 x 32 px the clip at 0 and at W / H cuts."""
    for H, W in ((96, 160), (32, 32)):
        b = DC.dfl_bias(bins)
        box = [np.broadcast_to(b[None, :, None, None], (1, 64, H // s, W // s)) for s in (8, 16, 32)]
        cls = [np.zeros((1, 1, H // s, W // s)) for s in (8, 16, 32)]
        ref = YR.decode(box, cls, H, W)[0, :, :4]
        want = DC.dfl_boxes(bins, H, W)
        assert np.isfinite(ref).all() and np.abs(ref - want).max() <= 1e-9, (bins, np.abs(ref - want).max())
        if 15 in bins:
            assert (want == 0).any() and ((want[:, 2] == W).any() or (want[:, 3] == H).any())
    sd = DC.dfl_net(bins)
    assert all(not sd[f"model.22.cv2.{l}.2.weight"].any() and np.array_equal(sd[f"model.22.cv2.{l}.2.bias"], b) for l in range(3))


def test_the_largest_shape_has_more_decode_blocks_than_the_scan_has_lanes():
    """k_yolo_decode_mb's last arriver scans the per-block candidates with 64 lanes: 448x448 is the smallest square frame at which a
    lane holds two (65 blocks), which is what tests/test_gpu_yolo_select.py runs its total ties at."""
    from openglottal_amd.yolo import YoloPlanner

    p = YoloPlanner(DC.base_sd())
    for (H, W), blocks in (((96, 160), 5), ((256, 256), 21), ((32, 32), 1), ((448, 448), 65)):
        assert (sum(DC.level_sizes(H, W)) + 63) // 64 == blocks
        for options, B, kernel, grid in (("", 1, "k_yolo_decode_mb", (blocks, 1)), ("latency_batch=8", 5, "k_yolo_decode_mb", (blocks, 5)),
                                         ("latency_batch=0", 5, "k_yolo_decode", (5, 1)), ("", 5, "k_yolo_decode", (5, 1))):
            r = p.plan(B, H, W, 256, options)[-1]
            assert (r["kernel"], r["module"], (r["gx"], r["gy"])) == (kernel, "model.22", grid), (H, W, options, r)
