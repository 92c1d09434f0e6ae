"""GPU (-m gpu): the detector's ``best`` row -- the step BEHIND the arithmetic -- on inputs where its branches fire.

The convolution launches are judged against float64 elsewhere; here the last 1x1 convs are set (tests/decode_cases.py) so that many
anchors share the largest confidence, every anchor does, the sigmoid saturates, the threshold IS a confidence, or the DFL softmax
sees one-hot, flat and +200 logits.  The expectation is ``decode_cases.select`` on the device's own ``pred`` (lowest index among the
largest confidences, strictly above the threshold, else ``(0,0,0,0,-1)``), exact closed forms, or the float64 decode of the device's
own logits.  Every case runs through both decode kernels, named from ``last_launches()``:

  k_yolo_decode_mb   calls of at most ``latency_batch`` frames: one-frame calls at the default, and 5 (or fewer) frames with
                     ``latency_batch`` 8, where blockIdx.y > 0
  k_yolo_decode      ``latency_batch`` 0, and calls of two or more frames at the default

at 96x160 (315 anchors: the last block of 64 is partial), 256x256 (1344 = 21 full blocks) and 32x32 (21 anchors: less than a block);
the total ties also at 448x448 (4116 anchors = 65 blocks: only past 64 blocks does a lane of the last arriver's scan hold two
candidates, so only there does the scan's own comparison decide -- a build with that comparison reversed passes every smaller shape).
The tie rule is written four times (the per-thread loop and the LDS tree of k_yolo_decode; the LDS tree, and the last arriver's
scan with its shuffle, of k_yolo_decode_mb): the tie nets put equal maxima in several 64-anchor blocks, levels and thread residues,
which the test asserts on the device's ``pred`` before it compares anything.
"""
import numpy as np
import pytest

import decode_cases as DC
from openglottal_amd._lib import check, lib, ptr
from openglottal_amd.yolo import YoloV8Detector, letterbox_bgr
from oracle import yolo_layer_ref as YR

pytestmark = pytest.mark.gpu

SHAPES = [(96, 160), (256, 256), (32, 32)]
# mode -> (latency_batch, one call per frame?, the decode kernel that must run)
MODES = {
    "mb: one-frame calls": (1, True, "k_yolo_decode_mb"),
    "mb: latency_batch 8": (8, False, "k_yolo_decode_mb"),
    "wg: latency_batch 0": (0, False, "k_yolo_decode"),
    "wg: batched call": (1, False, "k_yolo_decode"),
}
ONE = np.nextafter(np.float32(1), np.float32(2))
_dets = {}


def det(key, make_sd, precision="f32"):
    """One detector per (net, precision) and module; ``make_sd`` builds the state dict on first use."""
    k = (key, precision)
    if k not in _dets:
        d = YoloV8Detector(make_sd(), device="cuda:0", precision=precision)
        d.set_option("trace_launches", 1)
        _dets[k] = d
    return _dets[k]


def fresh(make_sd, precision="f32"):
    d = YoloV8Detector(make_sd(), device="cuda:0", precision=precision)
    d.set_option("trace_launches", 1)
    return d


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def decode_tolerance(H, W):   # as tests/test_gpu_yolo_launch_parity.py
    return 16 * float(np.spacing(np.float32(max(H, W)))), 8 * 2.0 ** -24


def run(d, fr, conf, mode, want_pred=True):
    """``(best [B,5], pred [B,A,5] | None)`` of ``fr`` through ``mode``; the decode kernel is read back from the launch trace."""
    lb, per_frame, kernel = MODES[mode]
    assert per_frame or lb == 0 or (len(fr) <= lb) == (kernel == "k_yolo_decode_mb"), (mode, len(fr))
    d.set_option("latency_batch", lb)
    try:
        outs = []
        for chunk in ([fr[i:i + 1] for i in range(len(fr))] if per_frame else [fr]):
            outs.append(d.detect_batch(chunk, conf=float(conf), want_pred=want_pred))
            ran = d.last_launches()
            assert ran[-1] == (kernel, "model.22"), (mode, ran[-1])
    finally:
        d.set_option("latency_batch", 1)
    if not want_pred:
        return np.concatenate(outs), None
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


def check_best(best, pred, thr, what):
    """``best`` is the oracle's row of the device's own ``pred``, bit for bit, for every frame; no NaN anywhere."""
    assert not np.isnan(pred).any() and not np.isnan(best).any(), what
    for b in range(len(pred)):
        want = DC.select(pred[b], thr)
        assert same_bits(best[b], want), (what, b, best[b], want, DC.tied(pred[b, :, 4])[:8])


def logits_of(d, B, H, W):
    cap = B * 64 * (H // 8) * (W // 8)
    return ([d.activation(f"model.22.cv2.{l}.2", B, cap=cap) for l in range(3)],
            [d.activation(f"model.22.cv3.{l}.2", B, cap=cap) for l in range(3)])


# ───────────────────────────── partial ties ─────────────────────────────


# (the 32x32 tie net's class weights, 2e-4 x 0.3, are subnormal in f16: the f16 mode runs the two larger shapes)
PARTIAL = [(s, "f32") for s in SHAPES] + [(s, "f16") for s in SHAPES[:2]]


@pytest.mark.parametrize("shape,precision", PARTIAL, ids=[f"{s[0]}x{s[1]}-{p}" for s, p in PARTIAL])
def test_partial_ties_lowest_index_of_the_largest_confidence_wins(shape, precision):
    H, W = shape
    c = DC.TIE_CASES[shape]
    d = det(("tie", c["scale"], c["bias"]), lambda: DC.tie_net(c["scale"], c["bias"]), precision)
    fr = DC.frames(H, W)
    got = {}
    for mode in MODES:
        best, pred = run(d, fr, 0.25, mode)
        st = DC.tie_stats(pred[:, :, 4], H, W)
        print(f"partial ties {H}x{W} {precision} [{mode}] {MODES[mode][2]}: {DC.describe(st)}")
        DC.check_tie_conditions(st, (shape, mode))                    # ... on the device's own pred, before anything is compared
        check_best(best, pred, 0.25, (shape, precision, mode))
        assert np.all(best[:, 4] > 0.25)
        got[mode] = (best, pred)
        if MODES[mode][0] == 1:   # without pred: the one-frame call writes `best` straight to the pinned buffer (zero copy)
            assert same_bits(run(d, fr, 0.25, mode, want_pred=False)[0], best), (shape, mode)
    # one-frame calls and the batched call: the same bits, winner included
    a, b = got["mb: one-frame calls"], got["wg: batched call"]
    assert same_bits(a[1], b[1]) and same_bits(a[0], b[0]), (shape, precision)


# ───────────────────────────── total ties, per-level biases, saturation ─────────────────────────────

MANY_BLOCKS = (448, 448)
TOTAL = [((0.0, 0.0, 0.0), 0), ((1.0, 0.0, 0.0), 0), ((0.0, 1.0, 0.0), 1), ((0.0, 0.0, 1.0), 2), ((100.0, 100.0, 100.0), 0)]


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("shape", SHAPES + [MANY_BLOCKS], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("biases,level", TOTAL, ids=[str(t[0]) for t in TOTAL])
def test_total_ties_the_first_anchor_of_the_highest_level_wins(biases, level, shape, precision):
    H, W = shape
    sizes = DC.level_sizes(H, W)
    winner = int(sum(sizes[:level]))
    n_tied = sum(s for s, b in zip(sizes, biases) if b == max(biases))
    d = det(("total", biases), lambda: DC.total_tie_net(biases), precision)
    fr = DC.frames(H, W, B=2 if shape == MANY_BLOCKS else 5, seed=11)
    for mode in MODES:
        best, pred = run(d, fr, 0.25, mode)
        boxl, clsl = logits_of(d, 1 if MODES[mode][1] else len(fr), H, W)
        conf = pred[:, :, 4]
        for b in range(len(fr)):
            t = DC.tied(conf[b])
            assert (int(t[0]), len(t)) == (winner, n_tied), (shape, mode, b, t[:4], len(t))
            assert same_bits(best[b], pred[b, winner]), (shape, mode, b, best[b], pred[b, winner])
        if biases[0] == 100.0:
            assert np.all(conf == np.float32(1.0))                   # saturation: exactly 1.0 everywhere, a total tie at 1.0
        check_best(best, pred, 0.25, (shape, precision, mode, biases))
        # the winner's box against the float64 decode of the device's own logits (of the frames the last call held)
        ref = YR.decode(boxl, clsl, H, W)
        rows = slice(len(fr) - 1, len(fr)) if MODES[mode][1] else slice(0, len(fr))
        tb, tc = decode_tolerance(H, W)
        eb = float(np.abs(best[rows, :4] - ref[:, winner, :4]).max())
        ec = float(np.abs(best[rows, 4] - ref[:, winner, 4]).max())
        assert eb <= tb and ec <= tc, (shape, mode, eb, ec)
        print(f"total tie {biases} {H}x{W} {precision} [{mode}] {MODES[mode][2]}: {n_tied} tied maxima in blocks "
              f"{winner // 64}..{(winner + n_tied - 1) // 64}, winner {winner}, max|dbox| {eb:.3g} px")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_saturation_at_zero_nothing_passes_conf_zero(shape):
    """Class bias -100: expf overflows to inf, conf is exactly 0, and at ``conf=0.0`` the strict > lets nothing pass."""
    H, W = shape
    d = det(("total", (-100.0,) * 3), lambda: DC.total_tie_net((-100.0,) * 3))
    fr = DC.frames(H, W, B=5, seed=11)
    for mode in MODES:
        best, pred = run(d, fr, 0.0, mode)
        assert np.all(bits(pred[:, :, 4]) == 0), (shape, mode)       # +0.0 exactly
        assert not np.isnan(pred).any()
        for b in range(len(fr)):
            assert same_bits(best[b], DC.NONE_ROW), (shape, mode, b, best[b])
        if MODES[mode][0] == 1:
            assert same_bits(run(d, fr, 0.0, mode, want_pred=False)[0], best)
        print(f"saturation at 0 {H}x{W} [{mode}] {MODES[mode][2]}: every conf +0.0, every row (0,0,0,0,-1)")


# ───────────────────────────── thresholds taken from pred itself ─────────────────────────────


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_thresholds_that_are_confidences(shape):
    H, W = shape
    c = DC.TIE_CASES[shape]
    d = det(("tie", c["scale"], c["bias"]), lambda: DC.tie_net(c["scale"], c["bias"]))
    fr = DC.frames(H, W)
    for mode in MODES:
        _, pred0 = run(d, fr, 0.25, mode)
        cs = np.unique(pred0[0, :, 4])[::-1]                          # frame 0's distinct confidences, descending
        assert len(cs) >= 2
        c0, c1 = np.float32(cs[0]), np.float32(cs[1])
        win = pred0[0, int(DC.tied(pred0[0, :, 4])[0])]
        for name, thr, want in (("c0", c0, DC.NONE_ROW), ("nextafter(c0, 0)", np.nextafter(c0, np.float32(0)), win), ("c1", c1, win),
                                ("0.0", np.float32(0), win), ("nextafter(1, 2)", ONE, DC.NONE_ROW)):
            best, pred = run(d, fr, thr, mode)
            assert same_bits(pred, pred0), (shape, mode, name)        # the threshold touches nothing but the selection
            assert same_bits(best[0], want), (shape, mode, name, best[0], want)
            check_best(best, pred, thr, (shape, mode, name))          # the other frames, whatever c0 is to them
            if MODES[mode][0] == 1:
                assert same_bits(run(d, fr, thr, mode, want_pred=False)[0], best), (shape, mode, name)
        print(f"thresholds {H}x{W} [{mode}] {MODES[mode][2]}: c0 {c0!r} c1 {c1!r}: none at c0, the c0 winner just below, at c1 and at 0")


# ───────────────────────────── state between launches on one handle ─────────────────────────────

def tie12():
    return DC.tie_net(0.3, 12.0)


# winner, none, other block counts (21, 65 -- a lane of the scan holds two --, 1), the first again
STEPS = [((96, 160), 0.25), ((96, 160), "c0"), ((256, 256), 0.25), ((448, 448), 0.25), ((32, 32), 0.25), ((96, 160), 0.25)]


def step_frames(shape):
    return DC.frames(*shape, B=3, seed=sum(shape))


@pytest.mark.parametrize("mode", list(MODES))
def test_state_between_launches_detect_batch(mode):
    """d_cand and d_dec_counter persist between launches: winner, nothing passes, other block counts, the first again -- each result
    equals a fresh handle's and the oracle's row of the call's own pred.  ("c0": the largest confidence of the three frames.)"""
    one, ref = fresh(tie12), det("tie12", tie12)
    got = []
    for shape, thr in STEPS:
        fr = step_frames(shape)
        t = np.float32(run(ref, fr, 0.25, mode)[1][:, :, 4].max()) if thr == "c0" else np.float32(thr)
        want = run(fresh(tie12), fr, t, mode, want_pred=False)[0]
        if thr == "c0":
            assert same_bits(want, np.tile(DC.NONE_ROW, (3, 1))), want
        else:
            assert np.all(want[:, 4] > 0.25)
        best = run(one, fr, t, mode, want_pred=False)[0]              # the one-frame calls of these: zero copy
        best_p, pred = run(one, fr, t, mode)
        check_best(best_p, pred, t, (mode, shape, thr))
        assert same_bits(best, best_p) and same_bits(best, want), (mode, shape, thr, best, want)
        got.append(best)
    assert same_bits(got[0], got[-1])
    print(f"state [{mode}] {MODES[mode][2]}: winner / none / 21, 65 and 1 blocks / winner again: each a fresh handle's bits")


def begin_end(d, fr, thr):
    B, H, W, _ = fr.shape
    f = np.ascontiguousarray(fr)
    check(lib().og_yolo_detect_u8_begin(d._h, ptr(f), B, H, W, float(thr)), "og_yolo_detect_u8_begin")
    best = np.empty((B, 5), np.float32)
    check(lib().og_yolo_detect_u8_end(d._h, ptr(best)), "og_yolo_detect_u8_end")
    return best


def test_state_between_launches_begin_end_zero_copy():
    """The same sequence through og_yolo_detect_u8_begin / _end, one frame per call: ``best`` is written to pinned memory by the
    kernel itself, the none row included."""
    one, ref = fresh(tie12), det("tie12", tie12)
    for shape, thr in STEPS:
        fr = step_frames(shape)
        for i in range(len(fr)):
            _, pred = run(ref, fr[i:i + 1], 0.25, "mb: one-frame calls")
            t = np.float32(pred[0, :, 4].max()) if thr == "c0" else np.float32(thr)
            want = DC.select(pred[0], t)
            assert (want[4] == -1) == (thr == "c0")
            got = begin_end(one, fr[i:i + 1], t)
            assert one.last_launches()[-1] == ("k_yolo_decode_mb", "model.22")
            assert same_bits(got[0], want), (shape, thr, i, got[0], want)
            if i == 0:
                assert same_bits(begin_end(fresh(tie12), fr[i:i + 1], t)[0], want)
    print("state [begin/end, zero copy] k_yolo_decode_mb: winner / none / 21, 65 and 1 blocks / winner again: each the oracle's row")


def scale_back(best, gain, px, py, H0, W0):
    """``YoloV8Detector.detect_frames_host``'s f32 scale-back of network-pixel rows (the specification of k_scale_boxes)."""
    best = best.copy()
    hit = best[:, 4] >= 0
    if (gain, px, py) != (1.0, 0, 0):
        best[:, [0, 2]] = (best[:, [0, 2]] - np.float32(px)) / np.float32(gain)
        best[:, [1, 3]] = (best[:, [1, 3]] - np.float32(py)) / np.float32(gain)
    best[:, [0, 2]] = best[:, [0, 2]].clip(0, W0)
    best[:, [1, 3]] = best[:, [1, 3]].clip(0, H0)
    best[~hit, :4] = 0
    return best.astype(np.float32)


@pytest.mark.parametrize("lb", [0, 1, 8])
def test_state_between_launches_resized_entry(lb):
    """The resident resized entry at letterboxes that are not the identity (k_letterbox_bgr -> chain -> decode -> k_scale_boxes): the
    none row must stay (0,0,0,0,-1) after k_scale_boxes, the winners are the oracle's rows scaled back."""
    import torch

    one, ref = fresh(tie12), det("tie12", tie12)
    kernel = "k_yolo_decode" if lb == 0 else "k_yolo_decode_mb"
    B = 1 if lb == 1 else 3
    for (H0, W0), thr in [((100, 120), 0.25), ((100, 120), "c0"), ((299, 500), 0.25), ((100, 120), 0.25)]:
        fr = np.random.RandomState(H0 + W0).randint(0, 256, (B, H0, W0, 3), dtype=np.uint8)
        lbx = [letterbox_bgr(f, 256) for f in fr]
        imgs, (gain, px, py) = np.stack([l[0] for l in lbx]), lbx[0][1:]
        assert imgs.shape[1:3] != (H0, W0) and (px or py)             # not the identity, and padded
        ref.set_option("latency_batch", lb)
        one.set_option("latency_batch", lb)
        try:
            best_n, pred = ref.detect_batch(imgs, conf=0.25, want_pred=True)
            t = np.float32(pred[:, :, 4].max()) if thr == "c0" else np.float32(thr)
            rows = np.stack([DC.select(p, t) for p in pred])
            assert np.all((rows[:, 4] == -1) == (thr == "c0"))
            want = scale_back(rows, gain, px, py, H0, W0)
            n0 = one.launch_count("k_scale_boxes")
            got = one.detect_resized_dev(torch.from_numpy(fr).to("cuda:0"), B, H0, W0, 3, float(t))
            assert one.launch_count("k_scale_boxes") == n0 + 1 and one.last_launches()[-1] == (kernel, "model.22")
        finally:
            ref.set_option("latency_batch", 1)
            one.set_option("latency_batch", 1)
        assert same_bits(got, want), ((H0, W0), thr, got, want)
        if thr == "c0":
            assert same_bits(got, np.tile(DC.NONE_ROW, (B, 1)))
    print(f"state [resized entry, latency_batch {lb}] {kernel}: winner / none / another shape / winner again through k_scale_boxes")


# ───────────────────────────── DFL extremes ─────────────────────────────

DFL_BINS = [(0, 0, 0, 0), (15, 15, 15, 15), (0, 15, 15, 0), (15, 0, 0, 15), (7.5, 7.5, 7.5, 7.5), ("+200",) * 4]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("bins", DFL_BINS, ids=str)
def test_dfl_extremes(bins, shape):
    """One-hot at bin 0 / 15 per side, all bins equal, +200 on every bin: ``pred`` boxes equal the closed form exactly (the clip at
    0 and at W / H included: 15 x 32 px exceeds every frame here) and the float64 decode of the device's own logits; no NaN."""
    H, W = shape
    d = det(("dfl", bins), lambda: DC.dfl_net(bins))
    fr = DC.frames(H, W, B=3, seed=5)
    want = DC.dfl_boxes(bins, H, W)
    for mode in MODES:
        best, pred = run(d, fr, 0.25, mode)
        nb = 1 if MODES[mode][1] else len(fr)
        boxl, clsl = logits_of(d, nb, H, W)
        assert all(np.array_equal(b, np.broadcast_to(DC.dfl_bias(bins)[None, :, None, None], b.shape)) for b in boxl)
        assert not np.isnan(pred).any() and not np.isnan(best).any(), (bins, shape, mode)
        ref = YR.decode(boxl, clsl, H, W)
        tb, tc = decode_tolerance(H, W)
        got = pred[len(fr) - nb:]
        eb, ec = float(np.abs(got[:, :, :4] - ref[:, :, :4]).max()), float(np.abs(got[:, :, 4] - ref[:, :, 4]).max())
        assert eb <= tb and ec <= tc, (bins, shape, mode, eb, ec)
        for b in range(len(fr)):
            assert same_bits(pred[b, :, :4], want), (bins, shape, mode, b, np.abs(pred[b, :, :4] - want).max())
        check_best(best, pred, 0.25, (bins, shape, mode))
        print(f"DFL {bins} {H}x{W} [{mode}] {MODES[mode][2]}: boxes equal the closed form exactly, max|dbox| against float64 {eb:.3g} px")
