"""The host side of include/openglottal_hip_gate.h and the Python on top of it, without a device: og_gate_select_host against numpy
and inside guard zones, the staged `area_waveform(skip_unboxed=True)` with a stub model and a scripted detector that record what
they were handed, `extract_gaw_features` against `_kinematic_features`, and the CLI's refusals."""
import numpy as np
import pytest

import buffer_guard as G
import gate_cases as GC
import openglottal_amd as og
from openglottal_amd import cli, features, gated
from openglottal_amd._lib import lib


@pytest.mark.parametrize("B", GC.SELECT_B)
def test_select_host_equals_numpy(B):
    for name, kept in GC.patterns(B).items():
        boxes = GC.boxes_for(kept)
        got = gated.select_host(boxes)
        assert got.dtype == np.int32 and np.array_equal(got, np.flatnonzero(kept)), (B, name)
        assert np.array_equal(got, GC.keep_of(boxes))


def test_the_rule_is_x1_at_least_zero_and_the_empty_slice_is_kept():
    boxes = np.array([[-1, -1, -1, -1], [0, 0, 0, 0], [0, 3, 9, 9], [-1, 5, 9, 9], [1, 1, 2, 2], [-2147483648, 0, 1, 1], [2147483647, 0, 1, 1]], np.int32)
    assert gated.select_host(boxes).tolist() == [1, 2, 4, 6]
    assert gated.select_host(np.zeros((0, 4), np.int32)).tolist() == []
    assert og.utils.normalize_box(None, 160, 96) == GC.NO_BOX            # what "no box" looks like in a boxes array


def test_select_host_stays_inside_its_extents():
    for B in (1, 257, 513):
        boxes = GC.boxes_for(GC.patterns(B)["all" if B == 1 else "random"])
        n = len(GC.keep_of(boxes))
        # keep is declared as the n entries the call writes: one more would show as a dirty guard
        out = G.run_guarded("og_gate_select_host", f"B={B}", lambda p: lib().og_gate_select_host(p["boxes"], B, p["keep"]),
                            {"boxes": boxes}, {"keep": 4 * n}, expect_rc=n)
        assert np.array_equal(out["keep"].view(np.int32), GC.keep_of(boxes))


# ── the staged pass ───────────────────────────────────────────────────────────────────────────────────────────────────
class ScriptedDetector:
    """`detect` returns the scripted box (or None) of the frame whose first pixel names it."""

    model = None                                              # no batched backend: `detect` is called frame by frame

    def __init__(self, boxes):
        self.boxes, self.seen, self.resets = boxes, [], 0

    def reset(self):
        self.resets += 1

    def detect(self, frame):
        i = int(frame.reshape(-1)[0])
        self.seen.append(i)
        b = self.boxes[i]
        return None if b[0] < 0 else tuple(int(v) for v in b)


class StubModel:
    """Records every frame it is handed; a frame's "area" is the sum of its pixels inside the box."""

    def __init__(self):
        self.calls = []

    def _areas(self, entry, run, boxes):
        self.calls.append((entry, [int(f.reshape(-1)[0]) for f in run]))
        out = np.zeros(len(run), np.int32)
        for j, f in enumerate(run):
            if boxes is None:
                out[j] = int(f.sum())
            elif boxes[j][0] >= 0:
                x1, y1, x2, y2 = boxes[j]
                out[j] = int(np.asarray(f)[y1:y2, x1:x2].sum())
        return None, out

    def segment_stream(self, run, threshold=0.5, boxes=None, **kw):
        return self._areas("stream", run, boxes)

    def segment_resized(self, run, net=256, threshold=0.5, boxes=None, want_mask=True, **kw):
        return self._areas("resized", run, boxes)


def _video(n, shape, seed):
    rs = np.random.RandomState(seed)
    fr = rs.randint(1, 256, (n,) + shape, dtype=np.uint8)
    fr.reshape(n, -1)[:, 0] = np.arange(n)                   # the frame's name
    return fr


@pytest.mark.parametrize("shape", [(12, 20), (12, 20, 3), (256, 256)])
@pytest.mark.parametrize("as_list", [False, True])
def test_the_staged_pass_hands_the_model_exactly_the_boxed_frames(monkeypatch, shape, as_list):
    monkeypatch.setattr(features, "BLOCK", 8)                 # three blocks of 8 frames and one of 6
    n = 30
    fr = _video(n, shape, 11)
    kept = GC.patterns(n)["random"].copy()
    kept[8:16] = False                                        # the second block has no box at all
    kept[16:24] = True                                        # the third has one on every frame
    boxes = GC.boxes_for(kept, shape[1], shape[0])
    src = list(fr) if as_list else fr
    m0, d0 = StubModel(), ScriptedDetector(boxes)
    want = features.area_waveform(src, d0, m0)
    m1, d1 = StubModel(), ScriptedDetector(boxes)
    got = features.area_waveform(src, d1, m1, skip_unboxed=True)
    assert got.dtype == np.float64 and np.array_equal(got, want) and want.max() > 0 and not want[~kept].any()
    assert d0.seen == d1.seen == list(range(n)) and d0.resets == d1.resets == 1
    entry = "stream" if shape[:2] == (256, 256) else "resized"
    assert [c[1] for c in m0.calls] == [list(range(lo, min(lo + 8, n))) for lo in range(0, n, 8)]      # the default: every frame
    per_block = [[i for i in range(lo, min(lo + 8, n)) if kept[i]] for lo in range(0, n, 8)]
    assert per_block[1] == [] and len(per_block[2]) == 8
    assert m1.calls == [(entry, blk) for blk in per_block if blk]                                        # boxed frames only, in order
    assert len(m1.calls) == 3                                                                            # the block without a box made no call
    # without a detector there is nothing to skip
    m2 = StubModel()
    assert np.array_equal(features.area_waveform(src, None, m2, skip_unboxed=True), features.area_waveform(src, None, StubModel()))
    assert sum(len(c[1]) for c in m2.calls) == n


def test_the_staged_pass_skips_inside_mixed_shapes(monkeypatch):
    a, b = _video(6, (12, 20), 1), _video(5, (10, 14, 3), 2)
    b.reshape(5, -1)[:, 0] += 6
    vid = list(a) + list(b)
    kept = np.array([1, 0, 1, 1, 0, 0, 0, 1, 0, 0, 1], bool)
    boxes = GC.boxes_for(kept, 14, 10)
    m0, m1 = StubModel(), StubModel()
    want = features.area_waveform(vid, ScriptedDetector(boxes), m0)
    got = features.area_waveform(vid, ScriptedDetector(boxes), m1, skip_unboxed=True)
    assert np.array_equal(got, want)
    assert [c[1] for c in m1.calls] == [[0, 2, 3], [7, 10]] and [c[1] for c in m0.calls] == [list(range(6)), list(range(6, 11))]


# ── extract_gaw_features ──────────────────────────────────────────────────────────────────────────────────────────────
def test_extract_gaw_features_is_kinematic_features_of_the_waveform_with_f0_in_hz(monkeypatch):
    t = np.arange(200)
    waves = {"periodic": np.round(500 + 400 * np.sin(2 * np.pi * t / 10.0)), "f0 None": np.concatenate([np.full(100, 10.0), np.full(100, 500.0)]),
             "silent": np.zeros(200)}
    assert og.extract_gaw_features is features.extract_gaw_features and "extract_gaw_features" in og.__all__
    for name, wave in waves.items():
        seen = {}

        def fake(frames, detector, model, device=None, **kw):
            seen.update(kw, resets=detector.resets)
            return wave.astype(np.float64)
        monkeypatch.setattr(features, "area_waveform", fake)
        det = ScriptedDetector(None)
        feats = features.extract_gaw_features(["frames"], 4000.0, det, object())
        assert seen == {"skip_unboxed": True, "resets": 1}, name              # reset first, then the kept-frames pass
        ref = features._kinematic_features([float(v) for v in wave])
        if name == "silent":
            assert feats is None and ref is None
            continue
        assert (ref["f0"] is None) == (name == "f0 None")
        assert feats["f0"] == (None if ref["f0"] is None else ref["f0"] * 4000.0)
        for k in ref:
            if k != "f0":
                assert np.array_equal(feats[k], ref[k]), (name, k)


# ── the CLI ───────────────────────────────────────────────────────────────────────────────────────────────────────────
def test_skip_unboxed_is_refused_outside_the_unet_pipeline(capsys):
    for argv in (["run", "v.npy", "--skip-unboxed", "--unet-weights", "u.pt"],                                   # run's default is unet-only
                 ["run", "v.npy", "--pipeline", "yolo-crop+unet", "--skip-unboxed", "--crop-weights", "c.pt", "--yolo-weights", "y.npz"],
                 ["run", "v.npy", "--pipeline", "guided-vft", "--skip-unboxed", "--yolo-weights", "y.npz"],
                 ["infer", "--input", "d", "--pipeline", "unet-only", "--skip-unboxed", "--unet-weights", "u.pt"],
                 ["infer", "--input", "d", "--pipeline", "guided-vft", "--skip-unboxed", "--yolo-weights", "y.npz"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2, argv
        assert "--skip-unboxed goes with --pipeline unet only" in capsys.readouterr().err, argv
    # with --pipeline unet the flag is accepted: the next refusal is about the weights
    for argv in (["run", "v.npy", "--pipeline", "unet", "--skip-unboxed", "--unet-weights", "u.pt"],
                 ["infer", "--input", "d", "--skip-unboxed", "--unet-weights", "u.pt"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and "--yolo-weights" in capsys.readouterr().err, argv
    import argparse

    ap = argparse.ArgumentParser()
    cli.add_infer_parser(ap.add_subparsers(dest="cmd"))
    assert ap.parse_args(["infer", "--input", "d"]).skip_unboxed is False and ap.parse_args(["infer", "--input", "d", "--skip-unboxed"]).skip_unboxed is True
