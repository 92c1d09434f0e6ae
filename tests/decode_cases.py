"""Detector nets whose LAST 1x1 convs are set so that the step behind the arithmetic -- the per-frame winner of ``k_yolo_decode`` /
``k_yolo_decode_mb`` -- takes the branches random weights never reach, and the selection rule those kernels are held to.

All builders are edits of ``synth.make_yolov8_state_dict(**YR.NETS["n"])``: only ``model.22.cv3.{l}.2`` (the class logit) and
``model.22.cv2.{l}.2`` (the 64 DFL logits) change, so every other launch is the net the parity tests judge.

* ``tie_net(scale, bias)``: class weight x ``scale``, class bias ``bias``.  A large bias puts every confidence where the f32 sigmoid is
  flat, so many distinct logits collapse onto ONE confidence: partial ties at whatever anchors the frame puts them.
* ``total_tie_net(biases)``: class weight x 0, one bias per level: every anchor of a level has the same confidence.  Equal biases: the
  winner is anchor 0; the largest bias on level l: the first anchor of that level.  +-100 saturate the sigmoid (1.0 / 0.0 exactly).
* ``dfl_net(bins)``: DFL weight x 0 with a bias that makes the distance of side s exactly ``bins[s]`` (an int: +80 on that bin; 7.5:
  all bins equal; ``"+200"``: +200 on every bin, 7.5 again, and inf / inf for a softmax without the max subtraction).

The tie rule (stated once, ``select``): of the anchors whose confidence is the frame's largest, the one with the LOWEST index wins, if
that confidence is ``> conf_thres`` (strict); otherwise the row is ``(0, 0, 0, 0, -1)``.
"""
import numpy as np

from openglottal_amd import synth
from oracle import yolo_layer_ref as YR

NET = "n"
NONE_ROW = np.array([0, 0, 0, 0, -1], np.float32)

# (H, W) -> class-branch scale and bias, frame seed, frames.  Chosen on the CPU emulation (tests/test_decode_cases.py prints what
# they give): 96x160 has 10-13 anchors at the maximum on two or three levels, 256x256 about 30, 32x32 (21 anchors, one block) 11-15.
# The weights of the first two stay normal f16 numbers (0.3 x 0.3), so the f16 mode sees the same collapse.
TIE_CASES = {
    (96, 160): dict(scale=0.3, bias=12.0, seed=1, B=5),
    (256, 256): dict(scale=0.3, bias=12.0, seed=2, B=2),
    (32, 32): dict(scale=2e-4, bias=5.0, seed=3, B=4),
}
MIN_TIED = 4   # anchors at the maximum, per frame


def base_sd() -> dict:
    return dict(synth.make_yolov8_state_dict(**YR.NETS[NET]))


def frames(H, W, B=None, seed=None):
    c = TIE_CASES.get((H, W), {})
    B = c.get("B", 3) if B is None else B
    seed = c.get("seed", H + W) if seed is None else seed
    return np.random.RandomState(seed).randint(0, 256, (B, H, W, 3), dtype=np.uint8)


def level_sizes(H, W):
    return [(H // s) * (W // s) for s in (8, 16, 32)]


def tie_net(scale, bias) -> dict:
    sd = base_sd()
    for l in range(3):
        k = f"model.22.cv3.{l}.2."
        sd[k + "weight"] = (sd[k + "weight"] * np.float32(scale)).astype(np.float32)
        sd[k + "bias"] = np.full_like(sd[k + "bias"], bias)
    return sd


def tie_net_for(H, W) -> dict:
    c = TIE_CASES[(H, W)]
    return tie_net(c["scale"], c["bias"])


def total_tie_net(biases=(0.0, 0.0, 0.0)) -> dict:
    sd = base_sd()
    for l in range(3):
        k = f"model.22.cv3.{l}.2."
        sd[k + "weight"] = np.zeros_like(sd[k + "weight"])
        sd[k + "bias"] = np.full_like(sd[k + "bias"], biases[l])
    return sd


def dfl_bias(bins) -> np.ndarray:
    b = np.zeros(64, np.float32)
    for s, q in enumerate(bins):
        if q == "+200":
            b[16 * s:16 * s + 16] = 200.0
        elif q != 7.5:
            b[16 * s + int(q)] = 80.0
    return b


def dfl_distance(q) -> float:
    return 7.5 if q in (7.5, "+200") else float(q)


def dfl_net(bins, sd=None) -> dict:
    """``bins``: (left, top, right, bottom).  The class branch stays the base net's (or ``sd``'s), so there is a winner to select."""
    sd = base_sd() if sd is None else dict(sd)
    for l in range(3):
        k = f"model.22.cv2.{l}.2."
        sd[k + "weight"] = np.zeros_like(sd[k + "weight"])
        sd[k + "bias"] = dfl_bias(bins)
    return sd


def dfl_boxes(bins, H, W) -> np.ndarray:
    """``[A,4]`` the closed form for integer / half-integer distances: ``clip((anchor -+ d) * stride)``, exact in f32 (every
    intermediate of the kernel's expression is a small multiple of 1/4)."""
    d = [dfl_distance(q) for q in bins]
    out = []
    for s in (8, 16, 32):
        h, w = H // s, W // s
        ay, ax = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        ax, ay = ax.reshape(-1), ay.reshape(-1)
        out.append(np.stack([((ax - d[0]) * s).clip(0, W), ((ay - d[1]) * s).clip(0, H),
                             ((ax + d[2]) * s).clip(0, W), ((ay + d[3]) * s).clip(0, H)], -1))
    return np.concatenate(out).astype(np.float32)


def select(pred, thr) -> np.ndarray:
    """THE selection oracle.  ``pred [A,5]`` f32 as the device wrote it, ``thr`` the call's ``conf_thres`` (compared as f32, as the
    kernel holds it): the row of the lowest index among those with the largest conf, if that conf > thr; else (0,0,0,0,-1)."""
    pred = np.asarray(pred, np.float32)
    conf = pred[:, 4]
    assert not np.isnan(conf).any()
    top = conf.max()
    if not top > np.float32(thr):
        return NONE_ROW.copy()
    return pred[int(np.flatnonzero(conf == top)[0])].copy()


def tied(conf) -> np.ndarray:
    conf = np.asarray(conf)
    return np.flatnonzero(conf == conf.max())


def tie_stats(conf, H, W) -> dict:
    """``conf [B,A]``: per frame the anchors at the maximum; over the batch the 64-anchor blocks (the workgroups of k_yolo_decode_mb
    and the LDS-tree leaves), the levels and the residues mod 256 (the threads of k_yolo_decode) they fall on."""
    ends = np.cumsum(level_sizes(H, W))
    sets = [tied(c) for c in np.asarray(conf)]
    every = np.concatenate(sets)
    return dict(per_frame=[len(s) for s in sets], first=[int(s[0]) for s in sets], blocks=sorted({int(i) // 64 for i in every}),
                levels=sorted({int(np.searchsorted(ends, i, side="right")) for i in every}), residues=len({int(i) % 256 for i in every}),
                distinct=[len(np.unique(c)) for c in np.asarray(conf)], A=int(np.asarray(conf).shape[1]))


def check_tie_conditions(st: dict, what=""):
    """What the GPU tie tests rely on: partial ties (not every anchor), several per frame, and -- where the frame has more than one
    block of 64 anchors -- spread over blocks, levels and thread residues, so that every one of the four comparisons decides."""
    assert min(st["per_frame"]) >= MIN_TIED, (what, st)
    assert max(st["per_frame"]) < st["A"], (what, st)          # partial: a total tie is another case
    assert len(st["levels"]) >= 2, (what, st)
    if st["A"] > 64:
        assert len(st["blocks"]) >= 2 and st["residues"] >= 2, (what, st)


def describe(st: dict) -> str:
    return (f"tied maxima per frame {st['per_frame']} of {st['A']} (first {st['first']}), blocks {st['blocks']}, levels {st['levels']}, "
            f"{st['residues']} residues mod 256, distinct confidences {st['distinct']}")
