"""`og_sweep_host` (include/openglottal_hip_sweep.h: the host twin of the device sweep, the same inline functions) against an independent
Python oracle (tests/sweep_cases.py: the Python state machine per configuration, numpy slicing), against the project's own tracker
entry column by column, against the reference's recorded traces and metrics, and inside guard-zoned buffers.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import buffer_guard as G
import sweep_cases as S
import track_cases as T
from openglottal_amd import gated, sweep
from openglottal_amd._lib import lib
from openglottal_amd.evaluate import metrics_from_counts

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("shape", S.SHAPES)
def test_the_host_twin_equals_the_python_oracle(shape, inclusive):
    for density in S.DENSITIES:
        o = S.oracle(shape, density, inclusive)
        got = sweep.sweep_host(o["pred"], o["gt"], o["best"], o["thresholds"], S.HOLDS, resets=o["resets"], inclusive=inclusive)
        assert np.array_equal(got["boxes"], o["boxes"]), (shape, density, np.argwhere((got["boxes"] != o["boxes"]).any(2))[:5])
        assert np.array_equal(got["frame_counts"], o["frame_counts"])
        assert np.array_equal(got["counts"], o["counts"]), (shape, density, np.argwhere((got["counts"] != o["counts"]).any(2))[:5])
    # the oracle itself saw boxes, held boxes and None, and at density 1 the counts are the box areas
    o = S.oracle(shape, 1.0, inclusive)
    det = o["counts"][:, :, 2]
    assert det.any() and not det.all()
    b = o["boxes"]
    assert np.array_equal(o["counts"][:, :, 1], np.where(b[:, :, 0] >= 0, (b[:, :, 2] - b[:, :, 0]) * (b[:, :, 3] - b[:, :, 1]), 0))
    assert (o["counts"][-len(S.HOLDS):, :, 2].sum(1) <= o["counts"][:len(S.HOLDS), :, 2].sum(1)).all()      # a higher threshold detects no more


@pytest.mark.parametrize("shape", S.SHAPES)
def test_a_threshold_equal_to_a_confidence_is_a_detection_only_under_the_inclusive_rule(shape):
    r = S.rows_for(shape)
    nh = len(S.HOLDS)
    hold0 = S.HOLDS.index(0)
    pred, gt = S.masks_for(shape, len(r["best"]), 0.5)
    det = {}
    for inclusive in (False, True):
        out = sweep.sweep_host(pred, gt, r["best"], r["thresholds"], S.HOLDS, resets=r["resets"], inclusive=inclusive, want_boxes=False)
        det[inclusive] = out["counts"][:, :, 2].reshape(len(r["thresholds"]), nh, -1)[:, hold0]        # [threshold, frame] at hold 0
    # every frame looked at follows a reset: no centre, so the gate alone decides
    for it, frame in ((1, r["own"][0]), (3, r["own"][1]), (2, r["half"])):
        assert float(r["best"][frame, 4]) == r["thresholds"][it]
        assert det[True][it, frame] == 1 and det[False][it, frame] == 0, (shape, it, frame)
    # 0.5 is the double 0.5: the f32 just above it is above it under both rules, and was not rounded down to it
    assert r["thresholds"][2] == 0.5 and r["best"][r["above"], 4] == S.JUST_ABOVE_HALF != np.float32(0.5)
    assert det[True][2, r["above"]] == 1 and det[False][2, r["above"]] == 1
    # a threshold given as the f32's double is NOT what (float)thr would be for 0.02-like values: the f64 0.02 is above f32(0.02)
    row = np.array([[0, 0, 1, 1, np.float32(0.02)]], np.float32)
    one = np.ones((1,) + shape, np.uint8)
    for inclusive in (False, True):
        out = sweep.sweep_host(one, one, row, [0.02, float(np.float32(0.02))], [0], inclusive=inclusive)
        assert out["counts"][:, 0, 2].tolist() == [0, int(inclusive)]


def test_every_column_equals_the_tracker_entry_on_pre_gated_rows():
    w = T.short_walk(400, 9, dict(max_shift_px=12.5, padding=3, max_hold_frames=0), (100, 120))
    best, resets, W, H = w["best"], w["resets"], w["W"], w["H"]
    thresholds, holds = [0.35, 0.5, 0.8], [0, 2, 7, S.FOREVER]
    pred, gt = S.masks_for((H, W), len(best), 0.5)
    for inclusive in (False, True):
        states = (gated.TrackState * 12)()
        out = sweep.sweep_host(pred, gt, best, thresholds, holds, resets=resets, max_shift_px=12.5, padding=3, inclusive=inclusive,
                               states=states)
        for it, thr in enumerate(thresholds):
            rows = best.copy()
            conf = rows[:, 4].astype(np.float64)
            rows[~((conf >= thr) if inclusive else (conf > thr)), 4] = -1
            for ih, hold in enumerate(holds):
                c = it * len(holds) + ih
                st = gated.TrackState()
                want = gated.track_host(st, gated.params_of(12.5, 3, hold), rows, W, H, resets)
                assert np.array_equal(out["boxes"][c], want), (inclusive, thr, hold)
                assert np.array_equal(out["counts"][c, :, 2], want[:, 0] >= 0)
                assert states[c].as_tuple() == st.as_tuple()
    # the states continue: two calls of 200 frames equal one of 400
    states = (gated.TrackState * 12)()
    a = sweep.sweep_host(pred[:200], gt[:200], best[:200], thresholds, holds, resets=resets[:200], max_shift_px=12.5, padding=3, states=states)
    b = sweep.sweep_host(pred[200:], gt[200:], best[200:], thresholds, holds, resets=resets[200:], max_shift_px=12.5, padding=3, states=states)
    whole = sweep.sweep_host(pred, gt, best, thresholds, holds, resets=resets, max_shift_px=12.5, padding=3)
    assert np.array_equal(np.concatenate([a["boxes"], b["boxes"]], 1), whole["boxes"])
    assert np.array_equal(np.concatenate([a["counts"], b["counts"]], 1), whole["counts"])


def test_the_host_twin_stays_inside_its_extents():
    for shape in ((1, 1), (7, 13), (33, 257)):
        o = S.oracle(shape, 0.5, False)
        n = 40
        H, W = shape
        thr = np.array(o["thresholds"], np.float64)
        hold = np.array(S.HOLDS, np.int32)
        Cn = len(thr) * len(hold)
        for with_boxes in (True, False):
            for with_resets in (True, False):
                out = G.run_guarded(
                    "og_sweep_host", f"{H}x{W} boxes={with_boxes} resets={with_resets}",
                    lambda p: lib().og_sweep_host(p["pred"], p["gt"], p["best"], p["resets"], n, H, W, p["thr"], len(thr), p["hold"], len(hold),
                                                  30.0, 8, 0, None, p["fc"], p["counts"], p["boxes"]),
                    {"pred": o["pred"][:n], "gt": o["gt"][:n], "best": o["best"][:n], "resets": o["resets"][:n] if with_resets else None,
                     "thr": thr, "hold": hold},
                    {"fc": n * 12, "counts": Cn * n * 12, "boxes": Cn * n * 16 if with_boxes else None})
                if with_resets:
                    assert np.array_equal(out["counts"].view(np.int32).reshape(Cn, n, 3), o["counts"][:, :n])
                    assert np.array_equal(out["fc"].view(np.int32).reshape(n, 3), o["frame_counts"][:n])
                    if with_boxes:
                        assert np.array_equal(out["boxes"].view(np.int32).reshape(Cn, n, 4), o["boxes"][:, :n])


def test_the_reference_traces_and_metrics():
    """tests/golden/sweep_traces.json (tests/golden/gen_golden_sweep.py): the reference's `TemporalDetector.detect` over one script
    for every (conf, hold) and its `frame_metrics` on masks regenerated from the recorded seed, held exactly."""
    with open(os.path.join(HERE, "golden", "sweep_traces.json")) as f:
        t = json.load(f)
    H, W = t["shape"]
    n = len(t["script"])
    rows = np.zeros((n, 5), np.float32)
    rows[:, 4] = -1
    for i, dets in enumerate(t["script"]):
        assert len(dets) <= 1
        if dets:
            rows[i] = dets[0]
    rs = np.random.RandomState(t["mask_seed"])
    pred = ((rs.rand(n, H, W) < t["mask_density"]) * 255).astype(np.uint8)
    gt = ((rs.rand(n, H, W) < t["mask_density"]) * 255).astype(np.uint8)
    out = sweep.sweep_host(pred, gt, rows, t["confs"], t["holds"], inclusive=False)
    unet_only = [metrics_from_counts(*r) for r in out["frame_counts"].tolist()]
    assert [list(m) for m in unet_only] == t["unet_only"]
    for it in range(len(t["confs"])):
        for ih in range(len(t["holds"])):
            c = it * len(t["holds"]) + ih
            rec = t["columns"][c]
            assert (rec["conf"], rec["hold"]) == (t["confs"][it], t["holds"][ih])
            got = [None if b[0] < 0 else list(b) for b in out["boxes"][c].tolist()]
            want = [None if b is None else [max(0, min(W, b[0])), max(0, min(H, b[1])), max(0, min(W, b[2])), max(0, min(H, b[3]))]
                    for b in rec["boxes"]]
            assert all(b is None or min(b) >= 0 for b in rec["boxes"])          # (no negative corner: a clamp is the whole normalisation)
            assert got == want, (rec["conf"], rec["hold"])
            m = [list(metrics_from_counts(tp, npred, ng)) for (tp, npred, _), (_, _, ng) in zip(out["counts"][c].tolist(), out["frame_counts"].tolist())]
            assert m == rec["metrics"], (rec["conf"], rec["hold"])
