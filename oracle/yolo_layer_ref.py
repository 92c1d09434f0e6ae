"""Float64 module-isolated references of the YOLOv8 detector and a per-element error bound.  TEST INFRASTRUCTURE.

Only ``tests/`` imports this module; nothing under ``openglottal_amd/`` does.

Each tapped module (``model.0`` .. ``model.21``, ``box*`` / ``cls*``) is recomputed in float64 from the GPU's OWN input taps,
with the op sequence of ``yolo_oracle`` (Conv = conv + BN (eps 1e-3) + SiLU, C2f, SPPF, nearest upsample, concat, the Detect
branches).  Upsample, concat and max-pool are exact.  Every value carries a bound, propagated through the module:

* a conv adds its own rounding ``kappa * 2^-24 * M`` with ``M = |s| * conv(|x|, |w|) + |s * mu| + |beta|`` (``kappa`` = the direct
  f32 MFMA form's, ``layer_ref.KAPPA["direct"]``) plus the SiLU's f32 evaluation (``4 * 2^-24 * |pre|``), and carries the bound of its
  input through ``|s| * conv(bound_in, |w|)`` times 1.1 (the largest slope of SiLU);
* SiLU is taken as the identity on magnitudes (|silu(v)| <= |v|);
* the C2f residual add adds the bounds of both operands and one rounding of ``|a| + |b|``;
* a max-pool's output error is at most the largest input error in its window.

``decode`` is the Detect head's decode (DFL softmax expectation, dist2bbox around the anchor centre, x stride, sigmoid, clip) in
float64 on the GPU's own ``box*`` / ``cls*`` logits, as ``yolo_oracle.forward`` / ``candidates`` compute it.
"""

from __future__ import annotations

import numpy as np

from .layer_ref import KAPPA, U
from .yolo_oracle import BN_EPS

SILU_SLOPE = 1.1     # max |d silu / dv| = 1.0998
SILU_ULPS = 4.0


def _t(v):
    import torch

    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))


class V:
    """A float64 value and its elementwise error bound (torch tensors)."""

    def __init__(self, v, e):
        self.v, self.e = v, e

    @staticmethod
    def exact(x):
        import torch

        x = _t(x) if isinstance(x, np.ndarray) else x.to(torch.float64)
        return V(x, torch.zeros_like(x))


def conv(x: V, sd: dict, p: str, s: int = 1, act: bool = True, kappa: float | None = None) -> V:
    import torch.nn.functional as F

    kappa = KAPPA["direct"] if kappa is None else kappa
    w = _t(sd[p + ".conv.weight"] if p + ".conv.weight" in sd else sd[p + ".weight"])
    k = w.shape[-1]
    if p + ".bn.weight" in sd:
        g, b = _t(sd[p + ".bn.weight"]), _t(sd[p + ".bn.bias"])
        mu, var = _t(sd[p + ".bn.running_mean"]), _t(sd[p + ".bn.running_var"])
        sc = g / (var + BN_EPS).sqrt()
        shift, aff = b - mu * sc, (sc * mu).abs() + b.abs()
    else:
        bias = _t(sd[p + ".conv.bias"] if p + ".conv.bias" in sd else sd[p + ".bias"])
        sc, shift, aff = bias * 0 + 1, bias, bias.abs()
    pre = sc[None, :, None, None] * F.conv2d(x.v, w, None, s, k // 2) + shift[None, :, None, None]
    M = sc.abs()[None, :, None, None] * F.conv2d(x.v.abs(), w.abs(), None, s, k // 2) + aff[None, :, None, None]
    e = kappa * U * M + sc.abs()[None, :, None, None] * F.conv2d(x.e, w.abs(), None, s, k // 2)
    if not act:
        return V(pre, e)
    return V(F.silu(pre), SILU_SLOPE * e + SILU_ULPS * U * pre.abs())


def cat(xs) -> V:
    import torch

    return V(torch.cat([x.v for x in xs], 1), torch.cat([x.e for x in xs], 1))


def up(x: V) -> V:
    import torch.nn.functional as F

    return V(F.interpolate(x.v, scale_factor=2.0, mode="nearest"), F.interpolate(x.e, scale_factor=2.0, mode="nearest"))


def maxpool5(x: V) -> V:
    import torch.nn.functional as F

    return V(F.max_pool2d(x.v, 5, 1, 2), F.max_pool2d(x.e, 5, 1, 2))


def c2f(x: V, sd: dict, p: str, shortcut: bool) -> V:
    y0 = conv(x, sd, p + ".cv1")
    c = y0.v.shape[1] // 2
    ys = [V(y0.v[:, :c], y0.e[:, :c]), V(y0.v[:, c:], y0.e[:, c:])]
    j = 0
    while f"{p}.m.{j}.cv1.conv.weight" in sd:
        z = conv(conv(ys[-1], sd, f"{p}.m.{j}.cv1"), sd, f"{p}.m.{j}.cv2")
        if shortcut:
            a = ys[-1]
            ys.append(V(a.v + z.v, a.e + z.e + U * (a.v.abs() + z.v.abs())))
        else:
            ys.append(z)
        j += 1
    return conv(cat(ys), sd, p + ".cv2")


def sppf(x: V, sd: dict) -> V:
    s = conv(x, sd, "model.9.cv1")
    y1 = maxpool5(s)
    y2 = maxpool5(y1)
    y3 = maxpool5(y2)
    return conv(cat([s, y1, y2, y3]), sd, "model.9.cv2")


def head_branch(f: V, sd: dict, pfx: str) -> V:
    h = conv(conv(f, sd, pfx + ".0"), sd, pfx + ".1")
    return conv(h, sd, pfx + ".2", act=False)


# module -> (inputs, fn(sd, *inputs)) ; "input" is the preprocessed frame (RGB / 255)
MODULES = {
    "model.0": (["input"], lambda sd, x: conv(x, sd, "model.0", 2)),
    "model.1": (["model.0"], lambda sd, x: conv(x, sd, "model.1", 2)),
    "model.2": (["model.1"], lambda sd, x: c2f(x, sd, "model.2", True)),
    "model.3": (["model.2"], lambda sd, x: conv(x, sd, "model.3", 2)),
    "model.4": (["model.3"], lambda sd, x: c2f(x, sd, "model.4", True)),
    "model.5": (["model.4"], lambda sd, x: conv(x, sd, "model.5", 2)),
    "model.6": (["model.5"], lambda sd, x: c2f(x, sd, "model.6", True)),
    "model.7": (["model.6"], lambda sd, x: conv(x, sd, "model.7", 2)),
    "model.8": (["model.7"], lambda sd, x: c2f(x, sd, "model.8", True)),
    "model.9": (["model.8"], lambda sd, x: sppf(x, sd)),
    "model.12": (["model.9", "model.6"], lambda sd, a, b: c2f(cat([up(a), b]), sd, "model.12", False)),
    "model.15": (["model.12", "model.4"], lambda sd, a, b: c2f(cat([up(a), b]), sd, "model.15", False)),
    "model.16": (["model.15"], lambda sd, x: conv(x, sd, "model.16", 2)),
    "model.18": (["model.16", "model.12"], lambda sd, a, b: c2f(cat([a, b]), sd, "model.18", False)),
    "model.19": (["model.18"], lambda sd, x: conv(x, sd, "model.19", 2)),
    "model.21": (["model.19", "model.9"], lambda sd, a, b: c2f(cat([a, b]), sd, "model.21", False)),
}
for _l, _f in enumerate(["model.15", "model.18", "model.21"]):
    MODULES[f"box{_l}"] = ([_f], lambda sd, x, _l=_l: head_branch(x, sd, f"model.22.cv2.{_l}"))
    MODULES[f"cls{_l}"] = ([_f], lambda sd, x, _l=_l: head_branch(x, sd, f"model.22.cv3.{_l}"))


def module(sd: dict, name: str, inputs: list) -> V:
    """Recompute one module from exact (GPU-tap) inputs: numpy arrays [B,C,H,W]."""
    return MODULES[name][1](sd, *[V.exact(x) for x in inputs])


def full_forward(sd: dict, x) -> dict:
    """Chain every module from the preprocessed input (float64, no taps): {name: V}.  Used on the CPU to pin the restatement
    to ``yolo_oracle.forward``."""
    out = {"input": V.exact(x)}
    for n, (ins, fn) in MODULES.items():
        out[n] = fn(sd, *[out[i] for i in ins])
    return out


def check_module(name: str, got: np.ndarray, ref: V, floor: float = 1e-30) -> float:
    """|got - ref| <= bound; returns the worst ratio, raises AssertionError naming the element otherwise."""
    r, e = ref.v.numpy(), ref.e.numpy() + floor
    assert got.shape == r.shape, (name, got.shape, r.shape)
    ratio = np.abs(got.astype(np.float64) - r) / e
    worst = float(ratio.max())
    if worst > 1.0:
        b, c, y, x = (int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        raise AssertionError(f"{name}: |err|/bound = {worst:.3g} at frame {b} ch {c} (y,x)=({y},{x}): got {got[b, c, y, x]!r} "
                             f"ref {r[b, c, y, x]!r} bound {e[b, c, y, x]:.3g}; {int((ratio > 1).sum())} element(s) over")
    return worst


def decode(boxes: list, clss: list, H: int, W: int) -> np.ndarray:
    """float64 decode of the Detect logits (box_l [B,64,h,w], cls_l [B,1,h,w]) -> [B,A,5] xyxy (clipped) + conf."""
    out = []
    for box, cls in zip(boxes, clss):
        box, cls = np.asarray(box, np.float64), np.asarray(cls, np.float64)
        B, _, h, w = box.shape
        stride = W / w
        lg = box.reshape(B, 4, 16, h * w)
        p = np.exp(lg - lg.max(2, keepdims=True))
        d = (p * np.arange(16)[None, None, :, None]).sum(2) / p.sum(2)          # [B,4,hw]
        sy, sx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
        ax, ay = sx.reshape(-1), sy.reshape(-1)
        x1, y1, x2, y2 = ax - d[:, 0], ay - d[:, 1], ax + d[:, 2], ay + d[:, 3]
        cx, cy = (x1 + x2) / 2 * stride, (y1 + y2) / 2 * stride
        ww, hh = (x2 - x1) * stride, (y2 - y1) * stride
        xyxy = np.stack([(cx - ww / 2).clip(0, W), (cy - hh / 2).clip(0, H), (cx + ww / 2).clip(0, W), (cy + hh / 2).clip(0, H)], -1)
        conf = 1.0 / (1.0 + np.exp(-cls[:, 0].reshape(B, h * w)))
        out.append(np.concatenate([xyxy, conf[..., None]], -1))
    return np.concatenate(out, 1)
