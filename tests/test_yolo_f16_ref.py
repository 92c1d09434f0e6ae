"""CPU: the float64 per-launch reference of the f16 detector (tests/yolo_f16_ref.py) judged on its own.

* the torch-CPU emulation of the f16 chain passes EVERY launch at kappa 16 on a scaled-down net, in both memory formats; the kappa it
  needs and the share of elements whose interval admits exactly one f16 value are recorded as named constants of the module;
* planted single-element mutants -- ten wrong ways to run one launch -- are each flagged AT the planted element;
* the end-to-end margins of tests/test_gpu_yolo_f16.py (E_BOX, E_CONF: the emulation's measured error against the f32 oracle on the
  test's own frames, the larger of the two memory formats) are re-measured here, and the oracle alone separates the top two
  confidences by more than 2 E_CONF on at least half of those frames.
"""
import numpy as np
import pytest

import yolo_f16_ref as R
from openglottal_amd import synth
from oracle import layer_ref as LR
from oracle import yolo_oracle as Y

SMALL = dict(seed=11, width=0.125)   # channels 8, 16, 32, 64, 128: model.2's 8-channel segments, every launch kind, seconds on a CPU


def small_case(B=2, H=192, W=256, seed=3):   # a 6 x 8 deepest map: the chained 5 x 5 pools differ from one another
    sd = synth.make_yolov8_state_dict(**SMALL)
    fr = np.random.RandomState(seed).randint(0, 256, (B, H, W, 3), dtype=np.uint8)
    return sd, Y.preprocess_bgr(fr).numpy()


@pytest.fixture(scope="module")
def emu():
    sd, x = small_case()
    return sd, R.device_weights(sd), {cl: R.emulate(sd, x, channels_last=cl) for cl in (False, True)}


def test_launch_list_names_every_stored_tensor_once():
    sd = synth.make_yolov8_state_dict(seed=7)
    names = R.tap_names(sd)
    assert len(names) == len(set(names))
    convs = {k[:-len(".conv.weight")] for k in sd if k.endswith(".conv.weight")} | {k[:-len(".weight")] for k in sd if k.endswith(".2.weight")}
    convs.discard("model.22.dfl")   # the DFL's arange(16) is part of the decode, not a stored tensor
    assert convs <= set(names), sorted(convs - set(names))
    assert {"model.9.m.1", "model.9.m.2", "model.9.m.3", "model.10", "model.13"} <= set(names)


def test_emulation_passes_every_launch_at_kappa_16(emu):
    sd, dw, both = emu
    worst, one, tot = {}, 0, 0
    for cl, taps in both.items():
        for spec in R.launches(sd):
            k = R.check_launch(spec, dw, taps)
            worst[spec["name"]] = max(worst.get(spec["name"], 0.0), k)
            a, b = R.sharp_share(spec, dw, taps)
            one, tot = one + a, tot + b
    top = max(worst.values())
    share = one / tot
    print("needed kappa per launch (max over NCHW / channels_last): " + " ".join(f"{k}={v:.2f}" for k, v in worst.items()))
    print(f"largest {top:.2f} of {R.KAPPA_F16:g}; the bound admits exactly one f16 value for {share:.4f} of {tot} stored elements")
    assert top <= R.KAPPA_F16
    assert top <= 2 * R.YOLO_F16_EMULATED_MAX, top
    assert share >= R.YOLO_F16_SHARP_SHARE, share


def pick(sd, pred):
    return next(s for s in R.launches(sd) if pred(s))


# mutant -> the launch it is planted in (scaled-down net: c(model.2) = 8 -> a lone half chunk at model.2.m.0.cv1)
TARGETS = {
    "store_trunc": lambda s: s["name"] == "model.4.m.0.cv1",
    "store_ulp_high": lambda s: s["name"] == "model.6.cv1",
    "weights_f32": lambda s: s["name"] == "model.8.m.0.cv1",
    "weights_trunc": lambda s: s["name"] == "model.12.cv2",
    "silu_of_rounded": lambda s: s["name"] == "model.15.m.0.cv2",
    "res_after_rounding": lambda s: s["name"] == "model.4.m.1.cv2",
    "half_chunk_dropped": lambda s: s["name"] == "model.2.m.0.cv1",
    "s2_tap_swapped": lambda s: s["name"] == "model.5",
    "pool_wrong_segment": lambda s: s["name"] == "model.9.m.2",
    "logits_f16": lambda s: s["name"] == "model.22.cv2.1.2",
}


@pytest.mark.parametrize("mut", R.MUTANTS)
def test_planted_single_element_mutant_is_flagged_at_the_planted_element(emu, mut):
    sd, dw, both = emu
    taps = dict(both[False])
    spec = pick(sd, TARGETS[mut])
    good = taps[spec["name"]]
    bad = R.emu_launch(spec, sd, dw, taps, mut=mut)
    ref, e, M = R.ref_launch(spec, dw, taps)
    # plant where the wrong value lies farthest outside what the check admits (a mutant that moves no element that far shows the
    # check too weak, and fails here)
    if e is None:
        score = np.abs(bad - good)
    elif spec["f32out"]:
        score = np.abs(bad.astype(np.float64) - ref) / LR.bound_of(M, R.KAPPA_F16)
    else:
        score = np.where(bad != good, LR.f16_needed(bad, ref) / e, 0.0)
    b, c, y, x = (int(v) for v in np.unravel_index(int(np.argmax(score)), score.shape))
    assert bad[b, c, y, x] != good[b, c, y, x], f"{mut} changes nothing in {spec['name']}"
    planted = good.copy()
    planted[b, c, y, x] = bad[b, c, y, x]
    taps[spec["name"]] = planted
    with pytest.raises(LR.LayerMismatch) as ei:
        R.check_launch(spec, dw, taps)
    msg = str(ei.value)
    assert spec["name"] in msg and f"frame {b} ch {c} (y,x)=({y},{x})" in msg, msg
    assert "1 element(s)" in msg, msg


def test_end_to_end_margins_and_oracle_separation():
    import test_gpu_yolo_f16 as G

    sd = synth.make_yolov8_state_dict(**G.E2E_WEIGHTS)
    fr = G.e2e_frames()
    ref = Y.candidates(sd, fr).astype(np.float64)
    eb = ec = 0.0
    for cl in (False, True):
        got = R.emulated_candidates(sd, fr, channels_last=cl)
        eb = max(eb, float(np.abs(got[..., :4] - ref[..., :4]).max()))
        ec = max(ec, float(np.abs(got[..., 4] - ref[..., 4]).max()))
    print(f"emulation against the f32 oracle on {len(fr)} frames: max|dbox| {eb:.4g} px, max|dconf| {ec:.4g}")
    assert eb <= G.E_BOX and ec <= G.E_CONF, (eb, ec)
    assert eb >= G.E_BOX / 2 and ec >= G.E_CONF / 2, ("the recorded margins are stale (more than 2x what the emulation shows)", eb, ec)
    top2 = np.sort(ref[..., 4], axis=1)[:, -2:]
    apart = (top2[:, 1] - top2[:, 0]) > 2 * G.E_CONF
    print(f"oracle: {int(apart.sum())} of {len(fr)} frames separate their top two confidences by more than 2 E_CONF")
    assert apart.sum() * 2 >= len(fr)
