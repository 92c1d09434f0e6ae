"""Float64 per-launch reference of the f16 detector (``og_yolo`` option ``"precision"`` 2) and a CPU emulation of it.
TEST INFRASTRUCTURE: the detector counterpart of ``oracle.layer_ref`` form ``"f16"``.

Every stored tensor of the chain -- each Conv's output by its module path, the three SPPF pools (``model.9.m.1..3``), the two
up-sampled maps (``model.10``, ``model.13``) and the Detect branches' convs -- is judged from its OWN input taps on the weights the
device holds (every MFMA conv's weights rounded to f16 once, ties to even; ``model.0`` and the folded BN pairs stay f32):

* a conv launch: ``pre = sc * conv(x, w) + shift`` in float64 and the magnitude pass ``M = |sc| conv(|x|, |w|) + |sc mu| + |beta|``
  as in ``oracle.yolo_layer_ref.conv``; the value before its one rounding carries
  ``e = kappa 2^-24 M + 4 2^-24 |pre|`` (SiLU evaluated in f32) ``+ 2^-24 (|a| + |z|)`` (the residual add), and the stored f16
  value must lie in ``[RNE16(ref - e), RNE16(ref + e)]`` (``layer_ref.check_f16``);
* the three f32 logit layers (``model.22.cv{2,3}.l.2``) take the plain magnitude check ``|got - ref| <= kappa 2^-24 M``;
* max-pools and up-sampling are exact on f16 values: bit equality.

``kappa = layer_ref.KAPPA["f16"] = 16``: the same MFMA, the same f32 accumulation as the U-Net's f16 mode.

The emulation (``emulate``) runs the same launches in torch f32 on the CPU, NCHW or ``channels_last``, rounding where the library
rounds; ``MUTANTS`` are wrong ways to run one launch, for tests/test_yolo_f16_ref.py to plant and the checks to flag.
"""

from __future__ import annotations

import numpy as np

from oracle import layer_ref as LR
from oracle.layer_ref import KAPPA, U
from oracle.yolo_layer_ref import A, affine, gather, launches, tap_names   # noqa: F401  (the chain's description: shared with the f32 reference)
from oracle.yolo_layer_ref import wkey as _wkey

KAPPA_F16 = KAPPA["f16"]
SILU_ULPS = 4.0
# recorded by tests/test_yolo_f16_ref.py::test_emulation_passes_every_launch_at_kappa_16 (asserts <= 2x this, and <= kappa)
YOLO_F16_EMULATED_MAX = 2.0
# share of elements whose interval [RNE16(ref - e), RNE16(ref + e)] holds exactly ONE f16 value (same test; asserts >= this)
YOLO_F16_SHARP_SHARE = 0.85   # measured 0.868


def device_weights(sd: dict) -> dict:
    """The tensors an f16-mode detector holds: the weights of every MFMA conv (all but ``model.0``) rounded to f16 once."""
    out = dict(sd)
    for k, v in sd.items():
        if np.ndim(v) == 4 and k.endswith(".weight") and not k.startswith("model.0.") and ".dfl." not in k:
            out[k] = np.asarray(v, np.float32).astype(np.float16).astype(np.float32)
    return out


def _t64(v):
    import torch

    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))


def ref_launch(spec: dict, dw: dict, taps: dict):
    """float64 reference of one launch from ITS OWN input taps -> (ref, e, M); e is None for the exact launches."""
    import torch.nn.functional as F

    x = gather(taps, spec["ins"]).astype(np.float64)
    if spec["op"] == "pool":
        return F.max_pool2d(_t64(x), 5, 1, 2).numpy(), None, None
    if spec["op"] == "up":
        return F.interpolate(_t64(x), scale_factor=2.0, mode="nearest").numpy(), None, None
    p = spec["name"]
    w = _t64(dw[_wkey(dw, p)])
    k = w.shape[-1]
    sc, sh, aff = affine(dw, p)
    sc64, sh64 = sc.astype(np.float64)[None, :, None, None], sh.astype(np.float64)[None, :, None, None]
    pre = sc64 * F.conv2d(_t64(x), w, None, spec["s"], k // 2).numpy() + sh64
    M = np.abs(sc64) * F.conv2d(_t64(np.abs(x)), w.abs(), None, spec["s"], k // 2).numpy() + aff[None, :, None, None]
    e = KAPPA_F16 * U * M
    ref = pre
    if spec["act"]:
        ref = pre / (1.0 + np.exp(-pre))
        e = e + SILU_ULPS * U * np.abs(pre)
    if spec["res"] is not None:
        a = gather(taps, [spec["res"]]).astype(np.float64)
        e = e + U * (np.abs(a) + np.abs(ref))
        ref = a + ref
    return ref, e + LR.FLOOR, M


def check_launch(spec: dict, dw: dict, taps: dict, frames=None) -> float:
    """Judge taps[spec.name] from its own input taps; returns the kappa the launch needed (0 for the exact launches)."""
    name, got = spec["name"], np.asarray(taps[spec["name"]])
    ref, e, M = ref_launch(spec, dw, taps)
    if e is None:
        LR.check_exact(name, got.astype(np.float64), ref, frames)
        return 0.0
    if spec["f32out"]:
        return KAPPA_F16 * LR.check(name, got, ref, LR.bound_of(M, KAPPA_F16), frames, tile=(8, 16))
    return LR.check_f16(name, got, ref, e, frames, tile=(8, 16), kappa=KAPPA_F16)


def sharp_share(spec: dict, dw: dict, taps: dict):
    """(elements whose interval admits exactly one f16 value, elements) of a stored conv launch."""
    ref, e, _ = ref_launch(spec, dw, taps)
    if e is None or spec["f32out"]:
        return 0, 0
    return int((LR.rne16(ref - e) == LR.rne16(ref + e)).sum()), int(ref.size)


# ───────────────────────────── CPU emulation (torch f32) ─────────────────────────────

MUTANTS = ("store_trunc", "store_ulp_high", "weights_f32", "weights_trunc", "silu_of_rounded", "res_after_rounding", "half_chunk_dropped",
           "s2_tap_swapped", "pool_wrong_segment", "logits_f16")


def _trunc16(v: np.ndarray) -> np.ndarray:
    """f32 -> f16 toward zero, as f32."""
    r = v.astype(np.float16)
    over = np.abs(r.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float32)


def emu_launch(spec: dict, sd: dict, dw: dict, taps: dict, channels_last: bool = False, mut: str | None = None) -> np.ndarray:
    """One launch as the library runs it, in torch f32: f16 operands (exact in f32), f32 accumulation, the f32 epilogue, one
    rounding.  ``mut``: one of MUTANTS (a wrong way to run this launch)."""
    import torch
    import torch.nn.functional as F

    def t(v):
        v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
        return v.contiguous(memory_format=torch.channels_last) if channels_last and v.ndim == 4 else v

    ins = spec["ins"]
    if spec["op"] == "pool":
        if mut == "pool_wrong_segment":
            ins = [A("model.9.cv1")]
        return F.max_pool2d(t(gather(taps, ins)), 5, 1, 2).numpy()
    if spec["op"] == "up":
        return F.interpolate(t(gather(taps, ins)), scale_factor=2.0, mode="nearest").numpy()
    p = spec["name"]
    w = np.asarray(dw[_wkey(dw, p)], np.float32)
    if mut == "weights_f32":
        w = np.asarray(sd[_wkey(sd, p)], np.float32)
    if mut == "weights_trunc":
        w = _trunc16(np.asarray(sd[_wkey(sd, p)], np.float32))
    if mut == "s2_tap_swapped":
        w = w.copy()
        w[:, :, 0, [1, 2]] = w[:, :, 0, [2, 1]]
    x = gather(taps, ins).astype(np.float32)
    if mut == "half_chunk_dropped":   # the last (half) 64-channel chunk of the padded input is never multiplied
        cp = (x.shape[1] + 31) // 32 * 32
        x = x.copy()
        x[:, (cp - 32):] = 0
    sc, sh, _ = affine(dw, p)
    with torch.no_grad():
        pre = F.conv2d(t(x), t(w), None, spec["s"], w.shape[-1] // 2) * t(sc)[None, :, None, None] + t(sh)[None, :, None, None]
        if mut == "silu_of_rounded":
            pre = pre.half().float()
        v = F.silu(pre) if spec["act"] else pre
        if spec["res"] is not None:
            a = t(gather(taps, [spec["res"]]).astype(np.float32))
            v = (v.half().float() + a) if mut == "res_after_rounding" else v + a
    v = v.contiguous().numpy()
    if spec["f32out"]:
        return v.astype(np.float16).astype(np.float32) if mut == "logits_f16" else v
    if mut == "store_trunc":
        return _trunc16(v)
    r = v.astype(np.float16)
    if mut == "store_ulp_high":
        r = np.nextafter(r, np.float16(np.inf))
    return r.astype(np.float32)


def emulate(sd: dict, x_input: np.ndarray, channels_last: bool = False) -> dict:
    """The whole chain: {tap name: [B,C,H,W] f32 holding f16 values (f32 logits for the three last layers)}."""
    dw = device_weights(sd)
    taps = {"input": np.asarray(x_input, np.float32)}
    for spec in launches(sd):
        taps[spec["name"]] = emu_launch(spec, sd, dw, taps, channels_last)
    return taps


def emulated_candidates(sd: dict, frames_bgr: np.ndarray, channels_last: bool = False) -> np.ndarray:
    """[B,A,5] xyxy + conf of the emulated f16 detector: float64 decode (``yolo_layer_ref.decode``) of its f32 logits."""
    from oracle import yolo_layer_ref as YR
    from oracle import yolo_oracle as Y

    taps = emulate(sd, Y.preprocess_bgr(frames_bgr).numpy(), channels_last)
    H, W = frames_bgr.shape[1:3]
    return YR.decode([taps[f"model.22.cv2.{l}.2"] for l in range(3)], [taps[f"model.22.cv3.{l}.2"] for l in range(3)], H, W)
