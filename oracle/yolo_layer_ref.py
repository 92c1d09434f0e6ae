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

from .layer_ref import FLOOR, KAPPA, U
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


def conv(x: V, sd: dict, p: str, s: int = 1, act: bool = True, kappa: float | None = None, folded=None) -> V:
    """``folded``: (scale, shift, |s mu| + |beta|) to use instead of the float64 fold of ``sd`` (``affine``: the device's f32 pair)."""
    import torch.nn.functional as F

    kappa = KAPPA["direct"] if kappa is None else kappa
    w = _t(sd[p + ".conv.weight"] if p + ".conv.weight" in sd else sd[p + ".weight"])
    k = w.shape[-1]
    if folded is not None:
        sc, shift, aff = (_t(v) for v in folded)
    elif p + ".bn.weight" in sd:
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


# ───────────────────────────── the chain launch by launch (both precisions) ─────────────────────────────


def A(name):
    return (name, None, None)


def launches(sd: dict) -> list:
    """The launches of one forward pass in execution order.  ``ins`` / ``res``: (tap name, first channel, end channel)."""
    L = []

    def conv(name, ins, s=1, act=True, res=None, f32out=False, first=False):
        L.append(dict(name=name, op="conv", ins=ins, s=s, act=act, res=res, f32out=f32out, first=first))

    def c2f(p, ins, shortcut):
        c = sd[p + ".cv1.conv.weight"].shape[0] // 2
        conv(p + ".cv1", ins)
        last = (p + ".cv1", c, 2 * c)
        cat = [(p + ".cv1", 0, 2 * c)]
        j = 0
        while f"{p}.m.{j}.cv1.conv.weight" in sd:
            conv(f"{p}.m.{j}.cv1", [last])
            conv(f"{p}.m.{j}.cv2", [A(f"{p}.m.{j}.cv1")], res=last if shortcut else None)
            last = A(f"{p}.m.{j}.cv2")
            cat.append(last)
            j += 1
        conv(p + ".cv2", cat)

    conv("model.0", [A("input")], 2, first=True)
    conv("model.1", [A("model.0")], 2)
    c2f("model.2", [A("model.1")], True)
    conv("model.3", [A("model.2.cv2")], 2)
    c2f("model.4", [A("model.3")], True)
    conv("model.5", [A("model.4.cv2")], 2)
    c2f("model.6", [A("model.5")], True)
    conv("model.7", [A("model.6.cv2")], 2)
    c2f("model.8", [A("model.7")], True)
    conv("model.9.cv1", [A("model.8.cv2")])
    prev = "model.9.cv1"
    for j in (1, 2, 3):
        L.append(dict(name=f"model.9.m.{j}", op="pool", ins=[A(prev)]))
        prev = f"model.9.m.{j}"
    conv("model.9.cv2", [A("model.9.cv1"), A("model.9.m.1"), A("model.9.m.2"), A("model.9.m.3")])
    L.append(dict(name="model.10", op="up", ins=[A("model.9.cv2")]))
    c2f("model.12", [A("model.10"), A("model.6.cv2")], False)
    L.append(dict(name="model.13", op="up", ins=[A("model.12.cv2")]))
    c2f("model.15", [A("model.13"), A("model.4.cv2")], False)
    conv("model.16", [A("model.15.cv2")], 2)
    c2f("model.18", [A("model.16"), A("model.12.cv2")], False)
    conv("model.19", [A("model.18.cv2")], 2)
    c2f("model.21", [A("model.19"), A("model.9.cv2")], False)
    for l, f in enumerate(["model.15.cv2", "model.18.cv2", "model.21.cv2"]):
        for br in ("cv2", "cv3"):
            p = f"model.22.{br}.{l}"
            conv(p + ".0", [A(f)])
            conv(p + ".1", [A(p + ".0")])
            conv(p + ".2", [A(p + ".1")], act=False, f32out=True)
    return L


def tap_names(sd: dict) -> list:
    return [s["name"] for s in launches(sd)]


def gather(taps: dict, ins) -> np.ndarray:
    return np.concatenate([np.asarray(taps[n])[:, lo:hi] for n, lo, hi in ins], 1)


def wkey(sd, p):
    return p + ".conv.weight" if p + ".conv.weight" in sd else p + ".weight"


def affine(sd: dict, p: str):
    """(scale, shift) as the device folds them (float64 arithmetic, each rounded to f32 once) and |s mu| + |beta|."""
    if p + ".bn.weight" in sd:
        g, b, mu, var = (np.asarray(sd[p + ".bn." + f], np.float64) for f in ("weight", "bias", "running_mean", "running_var"))
        s = g / np.sqrt(var + BN_EPS)
        return s.astype(np.float32), (b - mu * s).astype(np.float32), np.abs(s * mu) + np.abs(b)
    bk = p + ".conv.bias" if p + ".conv.bias" in sd else p + ".bias"
    b = np.asarray(sd[bk], np.float32) if bk in sd else np.zeros(sd[wkey(sd, p)].shape[0], np.float32)
    return np.ones_like(b), b, np.abs(b.astype(np.float64))


# ───────────────────────────── f32 mode (the default), launch by launch ─────────────────────────────
#
# Every stored tensor of the f32 chain is judged from ITS OWN input taps.  A conv launch is ``conv`` above on exact inputs, with the
# scale and shift the device holds (``affine``): value ``pre = sc conv(x, w) + sh`` (SiLU on top where the layer has one), bound
#   SILU_SLOPE * KAPPA["direct"] * 2^-24 * M + SILU_ULPS * 2^-24 * |pre|        (M = |sc| conv(|x|, |w|) + |sc mu| + |beta|)
# for the SiLU layers and ``KAPPA["direct"] * 2^-24 * M`` for the three logit layers of each branch, plus ``2^-24 (|a| + |z|)`` for
# the residual add of a shortcut bottleneck, plus ``layer_ref.FLOOR``.  No bound is carried from another launch: one launch, one
# rounding budget -- against ``check_module``, where a C2f's bound is pushed through its 4 to 10 convs.  Pools and up-sampling are
# exact.  With ``head_fused`` 1 the taps ``model.22.cv{2,3}.l.j`` are channel segments of the stacked chain's buffers and the
# reference is still the unstacked branch conv: a zero block that contributed anything would show here.

# largest kappa the torch-f32 CPU emulation (``emulate_f32``) needs over tests/test_yolo_layer_ref_f32.py's cases, NCHW and
# channels_last (that test asserts <= 2x this, and <= KAPPA["direct"])
YOLO_F32_EMULATED_MAX = 6.64   # channels_last, model.2.m.1.cv2 of the wider net at 480 x 512; the largest in NCHW is 4.52


def ref_launch_f32(spec: dict, sd: dict, taps: dict):
    """float64 reference of one f32-mode launch from ITS OWN input taps -> (ref, bound); bound is None for the exact launches."""
    import torch.nn.functional as F

    x = gather(taps, spec["ins"]).astype(np.float64)
    if spec["op"] == "pool":
        return F.max_pool2d(_t(x), 5, 1, 2).numpy(), None
    if spec["op"] == "up":
        return F.interpolate(_t(x), scale_factor=2.0, mode="nearest").numpy(), None
    z = conv(V.exact(x), sd, spec["name"], spec["s"], spec["act"], folded=affine(sd, spec["name"]))
    ref, e = z.v.numpy(), z.e.numpy()
    if spec["res"] is not None:
        a = gather(taps, [spec["res"]]).astype(np.float64)
        e = e + U * (np.abs(a) + np.abs(ref))
        ref = a + ref
    return ref, e + FLOOR


def check_launch_f32(spec: dict, sd: dict, taps: dict, frames=None) -> float:
    """Judge taps[spec.name] of an f32-mode run from that launch's own input taps; returns the kappa the launch needed (0 for the
    exact launches).  A failure (``layer_ref.LayerMismatch``) names the launch, frame, channel, pixel and 8 x 16 tile cell."""
    from .layer_ref import check, check_exact

    name, got = spec["name"], np.asarray(taps[spec["name"]])
    ref, e = ref_launch_f32(spec, sd, taps)
    if e is None:
        check_exact(name, got.astype(np.float64), ref, frames)
        return 0.0
    return KAPPA["direct"] * check(name, got, ref, e, frames, tile=(8, 16))


# torch-f32 CPU emulation of the f32 chain and wrong ways to run one launch of it (tests/test_yolo_layer_ref_f32.py)

MUTANTS_F32 = ("bn_eps_1e5", "last_chunk_dropped", "k_part_dropped", "s2_taps_swapped", "res_wrong_half", "head_zero_block_filled",
               "pool_wrong_segment", "up_shifted", "operands_10bit", "weights_f16", "silu_of_f16")


def _trunc10(v: np.ndarray) -> np.ndarray:
    """f32 with the mantissa cut to 10 bits (toward zero)."""
    return (np.ascontiguousarray(v, np.float32).view(np.uint32) & np.uint32(0xFFFFE000)).view(np.float32)


def emu_launch_f32(spec: dict, sd: dict, taps: dict, channels_last: bool = False, mut: str | None = None) -> np.ndarray:
    """One launch as the library runs it, in torch f32 on the CPU: f32 operands and sums, the folded f32 scale and shift, SiLU and the
    residual add in f32.  ``mut``: one of MUTANTS_F32."""
    import torch
    import torch.nn.functional as F

    def t(v):
        v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
        return v.contiguous(memory_format=torch.channels_last) if channels_last and v.ndim == 4 else v

    ins = spec["ins"]
    if spec["op"] == "pool":
        if mut == "pool_wrong_segment":
            ins = [A("model.9.cv1")]
        return F.max_pool2d(t(gather(taps, ins)), 5, 1, 2).contiguous().numpy()
    if spec["op"] == "up":
        v = F.interpolate(t(gather(taps, ins)), scale_factor=2.0, mode="nearest").contiguous().numpy()
        return np.roll(v, 1, axis=3) if mut == "up_shifted" else v
    p = spec["name"]
    w = np.asarray(sd[wkey(sd, p)], np.float32)
    x = gather(taps, ins).astype(np.float32)
    sc, sh, _ = affine(sd, p)
    if mut == "bn_eps_1e5":
        g, b, mu, var = (np.asarray(sd[p + ".bn." + f], np.float64) for f in ("weight", "bias", "running_mean", "running_var"))
        s64 = g / np.sqrt(var + 1e-5)
        sc, sh = s64.astype(np.float32), (b - mu * s64).astype(np.float32)
    if mut == "s2_taps_swapped":
        w = w.copy()
        w[:, :, 0, [1, 2]] = w[:, :, 0, [2, 1]]
    if mut == "last_chunk_dropped":   # the last 32-channel chunk of the padded input is never multiplied
        x = x.copy()
        x[:, ((x.shape[1] + 31) // 32 * 32 - 32):] = 0
    if mut == "k_part_dropped":       # one K part of a split never reaches the sum: the first quarter of the input channels
        w = w.copy()
        w[:, : max(1, w.shape[1] // 4)] = 0
    if mut == "operands_10bit":
        x, w = _trunc10(x), _trunc10(w)
    if mut == "weights_f16":
        w = w.astype(np.float16).astype(np.float32)
    res = spec["res"]
    if mut == "res_wrong_half":
        n, lo, hi = res
        assert lo is not None and lo > 0, "plant this one at a C2f's first bottleneck"
        res = (n, 0, lo)
    with torch.no_grad():
        acc = F.conv2d(t(x), t(w), None, spec["s"], w.shape[-1] // 2)
        if mut == "head_zero_block_filled":   # the stacked head's zero block holds the other branch's weights
            other = p.replace(".cv2.", ".cv3.") if ".cv2." in p else p.replace(".cv3.", ".cv2.")
            wo = np.asarray(sd[wkey(sd, other)], np.float32)
            xo = np.asarray(taps[other[:-1] + str(int(other[-1]) - 1)], np.float32)
            wo = wo[np.arange(w.shape[0]) % wo.shape[0]]
            acc = acc + F.conv2d(t(xo), t(wo), None, 1, wo.shape[-1] // 2)
        pre = acc * t(sc)[None, :, None, None] + t(sh)[None, :, None, None]
        if mut == "silu_of_f16":
            pre = pre.half().float()
        v = F.silu(pre) if spec["act"] else pre
        if res is not None:
            v = v + t(gather(taps, [res]).astype(np.float32))
    return v.contiguous().numpy()


def emulate_f32(sd: dict, x_input: np.ndarray, channels_last: bool = False) -> dict:
    """The whole f32 chain: {tap name: [B,C,H,W] f32}."""
    taps = {"input": np.asarray(x_input, np.float32)}
    for spec in launches(sd):
        taps[spec["name"]] = emu_launch_f32(spec, sd, taps, channels_last)
    return taps


def chain_refs(sd: dict, x_input) -> dict:
    """The launch references chained from the preprocessed input in float64 (no taps): {tap name: float64 [B,C,H,W]}."""
    taps = {"input": np.asarray(x_input, np.float64)}
    for spec in launches(sd):
        taps[spec["name"]] = ref_launch_f32(spec, sd, taps)[0]
    return taps


# ───────────────────────────── the f32 kernel list and the GPU matrix (tests/test_gpu_yolo_launch_parity.py) ─────────────────────────────

NETS = {"n": dict(seed=7), "w375": dict(seed=11, width=0.375, depth=0.67), "w125": dict(seed=11, width=0.125)}


def plan_labels(recs) -> list:
    """The launches of an og_yolo_plan record list (or of ``YoloV8Detector.last_launches``: (label, module) pairs) by instantiation:
    the label with what names no other code path dropped (`` cq_shift=N``, `` vsplit=N`` -- the template argument VS says it --,
    `` ksplit=1``) and `` ksplit=N``, N > 1, as ``+splitK+reduce`` (the fused reduce: the only split the detector's f32 chain takes)."""
    import re

    out = []
    for r in recs:
        k = r["kernel"] if isinstance(r, dict) else r[0]
        k = re.sub(r" (cq_shift|vsplit)=\d+", "", k)
        m = re.search(r" ksplit=(\d+)", k)
        if m:
            k = k[:m.start()] + ("" if int(m.group(1)) == 1 else "+splitK+reduce") + k[m.end():]
        out.append(k)
    return out


def module_map(module: str, H: int, W: int):
    """(h, w) of the map a launch serving ``module`` writes, for H x W frames."""
    p = module.split(".")
    i = int(p[1].split("-")[0])
    if i == 22:
        s = 8 << int(p[3]) if len(p) > 3 else 8
    else:
        s = {0: 2, 1: 4, 2: 4, 3: 8, 4: 8, 5: 16, 6: 16, 7: 32, 8: 32, 9: 32, 10: 16, 12: 16, 13: 8, 15: 8, 16: 16, 18: 16, 19: 32, 21: 32}[i]
    return H // s, W // s


def has_partial_tile(rec: dict, H: int, W: int) -> bool:
    """Does this MFMA conv launch (8 x 16 pixel tiles) have a tile that crosses the map's edge?"""
    h, w = module_map(rec["module"], H, W)
    return bool(h % 8 or w % 16)


# Every instantiation the f32 detector chain (``y_launch`` and the launch sites of ``YNet`` in og_yolo.inc) can launch, by a short label
# -> (its text as ``plan_labels`` reads og_yolo_plan, a smallest (net of NETS, H, W, B, options) that reaches it with a tile that
# crosses the map's edge).  tests/test_yolo_layer_ref_f32.py closes the list on the CPU at 256 CUs: the option sweep finds no label
# outside it, every entry is reached by its own case, and GPU_ROWS below together run every one of them on a shape with partial tiles.
# (k_conv_direct<false, *> -- stride-2 convs on the VALU kernel -- had no reachable switch and is gone from the launch code.)
YOLO_F32_KERNELS = {
    "direct<true,1>": ("k_conv_direct<true, 1>", ('w125', 32, 32, 1, '')),
    "direct<true,4>": ("k_conv_direct<true, 4>", ('w125', 32, 32, 1, 'latency_batch=0')),
    "o<1,0,8,3>": ("k_conv_mfma_o<1, 0, 8, 3, false, false>", ('w125', 96, 160, 48, 'splitk_max=1')),
    "o<1,0,8,3>+splitK+reduce": ("k_conv_mfma_o<1, 0, 8, 3, false, false>+splitK+reduce", ('w125', 32, 32, 1, '')),
    "o<1,0,8,3,VS>": ("k_conv_mfma_o<1, 0, 8, 3, false, true>", ('w125', 32, 32, 1, 'latency_batch=0')),
    "o<1,2,8,3>": ("k_conv_mfma_o<1, 2, 8, 3, false, false>", ('w125', 32, 32, 64, 'splitk_max=1,latency_batch=64')),
    "o<1,2,8,3>+splitK+reduce": ("k_conv_mfma_o<1, 2, 8, 3, false, false>+splitK+reduce", ('w125', 32, 32, 1, '')),
    "o<1,2,8,3,VS>": ("k_conv_mfma_o<1, 2, 8, 3, false, true>", ('w125', 32, 32, 1, 'latency_batch=0')),
    "o<1,3,8,3>": ("k_conv_mfma_o<1, 3, 8, 3, false, false>", ('w125', 32, 32, 1, 'splitk_max=1')),
    "o<1,3,8,3>+splitK+reduce": ("k_conv_mfma_o<1, 3, 8, 3, false, false>+splitK+reduce", ('w125', 32, 32, 1, '')),
    "o<1,3,8,3,VS>": ("k_conv_mfma_o<1, 3, 8, 3, false, true>", ('w125', 32, 32, 1, 'latency_batch=0')),
    "o<2,0,8,3>": ("k_conv_mfma_o<2, 0, 8, 3, false, false>", ('n', 96, 160, 48, 'splitk_max=1')),
    "o<2,0,8,3>+splitK+reduce": ("k_conv_mfma_o<2, 0, 8, 3, false, false>+splitK+reduce", ('w125', 32, 32, 1, 'latency_nt1=0')),
    "o<2,0,8,3,VS>": ("k_conv_mfma_o<2, 0, 8, 3, false, true>", ('w125', 32, 32, 1, 'latency_batch=0')),
    "o<2,2,8,3>": ("k_conv_mfma_o<2, 2, 8, 3, false, false>", ('w125', 96, 160, 48, '')),
    "o<2,2,8,3>+splitK+reduce": ("k_conv_mfma_o<2, 2, 8, 3, false, false>+splitK+reduce", ('w125', 32, 32, 1, 'latency_nt1=0')),
    "o<2,2,8,3,VS>": ("k_conv_mfma_o<2, 2, 8, 3, false, true>", ('w125', 32, 32, 1, 'latency_batch=0')),
    "o<2,3,8,3>": ("k_conv_mfma_o<2, 3, 8, 3, false, false>", ('w125', 32, 32, 1, 'splitk_max=1,latency_batch=0')),
    "o<2,3,8,3>+splitK+reduce": ("k_conv_mfma_o<2, 3, 8, 3, false, false>+splitK+reduce", ('w125', 32, 32, 1, 'latency_nt1=0')),
    "o<2,3,8,3,VS>": ("k_conv_mfma_o<2, 3, 8, 3, false, true>", ('w125', 32, 32, 1, 'latency_batch=0')),
    "p<1,0,8,3>": ("k_conv_mfma_p<1, 0, 8, 3>", ('w125', 32, 32, 1, 'splitk_max=1')),
    "p<1,2,8,1>": ("k_conv_mfma_p<1, 2, 8, 1>", ('w125', 32, 32, 1, '')),
    "p<2,0,8,1>": ("k_conv_mfma_p<2, 0, 8, 1>", ('w125', 32, 32, 1, 'splitk_max=1,latency_batch=0')),
    "p<2,2,8,1>": ("k_conv_mfma_p<2, 2, 8, 1>", ('w125', 32, 32, 1, 'latency_nt1=0')),
    "maxpool5": ("k_maxpool5", ('w125', 32, 32, 1, 'latency_batch=0')),
    "sppf_pools": ("k_sppf_pools", ('w125', 32, 32, 1, '')),
    "upsample2": ("k_upsample2", ('w125', 32, 32, 1, '')),
    "yolo_decode": ("k_yolo_decode", ('w125', 32, 32, 1, 'latency_batch=0')),
    "yolo_decode_mb": ("k_yolo_decode_mb", ('w125', 32, 32, 1, '')),
}

# label -> the rule in og_yolo.inc that keeps it from a shape with partial tiles (none needed: every entry has an edge row).  One PATH,
# not an instantiation, stays unjudged on the GPU: k_yolo_decode for a one-frame call, which YNet::decode takes only when
# (anchors + 63) / 64 > og_yolo::kDecBlocks = 512, i.e. for more than 32 768 anchors (a 1600 x 1600 frame); batched rows run the kernel.
YOLO_EDGE_EXEMPT = {}


def _row(net, H, W, B, options="", judge=None):
    rid = f"{net}-{H}x{W}-B{B}" + ("-" + options.replace(",", "-").replace("=", "") if options else "")
    return dict(id=rid, net=net, H=H, W=W, B=B, options=options, judge=judge)


# The GPU matrix: (net, H, W, B, options); ``judge``: how many frames are read back and judged (default: first two, middle, last).
GPU_ROWS = [
    _row("n", 96, 160, 1), _row("n", 96, 160, 2), _row("n", 96, 160, 48),
    _row("n", 160, 256, 1), _row("n", 160, 256, 2),          # 5 x 8 deepest map: half-row clipping
    _row("n", 32, 32, 1), _row("n", 32, 32, 3),              # 1 x 1 deepest map
    _row("n", 480, 512, 1),                                  # 15 x 16 = 240 > 224 pixels: k_maxpool5 on the latency path
    _row("n", 384, 384, 64, "latency_batch=64", judge=4),    # a real split no longer fits 4096 counters: the virtual split on the latency path
    _row("n", 96, 160, 2, "splitk_max=1"), _row("n", 96, 160, 48, "splitk_max=1"),   # every un-split form
    _row("n", 96, 160, 1, "latency_nt1=0"),
    _row("n", 96, 160, 1, "head_fused=0"), _row("n", 96, 160, 2, "head_fused=0"),
    _row("n", 96, 160, 3, "latency_batch=4"), _row("n", 96, 160, 1, "latency_batch=0"),
    _row("n", 96, 160, 1, "splitk_min_steps=9,splitk_max=2"),
    _row("n", 96, 160, 1, "splitk_slots=4,splitk_div=1,splitk_min_steps=1,splitk_max=64"),
    _row("n", 96, 160, 2, "splitk_slots=4,splitk_div=1,splitk_min_steps=1,splitk_max=64"),
    _row("w375", 96, 160, 1), _row("w375", 96, 160, 2), _row("w375", 96, 160, 48),   # 160 stacked head channels: NT = 1 with 5 column tiles; 4 bottlenecks
    _row("w375", 160, 256, 1), _row("w375", 96, 160, 1, "latency_nt1=0"),
]

# Rows that are the ONLY cover of no instantiation (overall or among the rows where it has a partial tile): what each adds instead.
# tests/test_yolo_layer_ref_f32.py holds this set exact, so that dropping any OTHER row fails by the name of the instantiation lost.
YOLO_REDUNDANT_FOR_COVERAGE = {
    "n-96x160-B1": "the default one-frame call on the edge shape: real split-K with the fused reduce at every layer, k_sppf_pools, k_yolo_decode_mb",
    "n-96x160-B2": "the default batched call at the smallest batch: the virtual split of the same K parts (bits compared with B = 1)",
    "n-96x160-B48": "a batch that fills the chip: grid.z frame groups, the occupancy kernel for model.2.cv1",
    "n-160x256-B1": "5 x 8 deepest map: a tile clipped in the middle of its rows, one-frame kernels",
    "n-160x256-B2": "5 x 8 deepest map, batched kernels",
    "n-32x32-B1": "1 x 1 deepest map: every tile of every MFMA launch is partial, the pools see padding only",
    "n-32x32-B3": "1 x 1 deepest map, batched, an odd batch",
    "n-480x512-B1": "15 x 16 = 240 > 224 pixels: the one-frame call takes k_maxpool5 three times; 1920 + 480 + 240 anchors in k_yolo_decode_mb",
    "n-384x384-B64-latency_batch64": "64 frames on the latency path: real splits that no longer fit the 4096 arrival counters fall back to the virtual split",
    "n-96x160-B2-splitk_max1": "the un-split persistent and stride-2 forms at a batch that does not fill the chip",
    "n-96x160-B1-latency_nt10": "64-column tiles on the latency path: the NT = 2 real splits",
    "n-96x160-B1-head_fused0": "the six Detect branch chains instead of the stacked one, one-frame kernels",
    "n-96x160-B2-head_fused0": "the six Detect branch chains, batched kernels",
    "n-96x160-B3-latency_batch4": "three frames on the latency path: arrival counters and workspace indexed by frame",
    "n-96x160-B1-latency_batch0": "a one-frame call on the batched kernels",
    "n-96x160-B1-splitk_min_steps9-splitk_max2": "two K parts of whole chunks: another summation order",
    "n-96x160-B1-splitk_slots4-splitk_div1-splitk_min_steps1-splitk_max64": "the finest split the options allow (K parts of one (chunk, tap) step), real",
    "n-96x160-B2-splitk_slots4-splitk_div1-splitk_min_steps1-splitk_max64": "the finest split, virtual: the most register-held parts",
    "w375-96x160-B1": "the wider, deeper net: 24/48/96/192/384 channels (padded segments of 24 and 48), 4 bottlenecks, 160 stacked head channels (NT = 1, 5 column tiles)",
    "w375-96x160-B2": "the wider net, batched",
    "w375-96x160-B48": "the wider net at a batch that fills the chip",
    "w375-160x256-B1": "the wider net on the 5 x 8 deepest map",
    "w375-96x160-B1-latency_nt10": "the wider net's NT = 2 real splits",
}

# largest kappa needed on one MI355X (256 CUs) per kernel family and net over GPU_ROWS, as tests/test_gpu_yolo_launch_parity.py
# prints it.  Recorded, not asserted: the gate is KAPPA["direct"] = 16.
YOLO_F32_GPU_MAX = {
    ("direct", "n"): 3.42, ("o MODE 0", "n"): 3.18, ("o MODE 2", "n"): 3.58, ("o MODE 3", "n"): 3.48,
    ("o MODE 0 VS", "n"): 2.53, ("o MODE 2 VS", "n"): 2.37, ("o MODE 3 VS", "n"): 2.93,
    ("o MODE 0 splitK+reduce", "n"): 2.23, ("o MODE 2 splitK+reduce", "n"): 2.61, ("o MODE 3 splitK+reduce", "n"): 2.43,
    ("persistent MODE 0", "n"): 3.81, ("persistent MODE 2", "n"): 3.09,
    ("k_maxpool5", "n"): 0.0, ("k_sppf_pools", "n"): 0.0, ("k_upsample2", "n"): 0.0,
    # the 0.375 / 0.67 net (its rows take the split forms only: the un-split ones are judged on the n net)
    ("direct", "w375"): 3.22, ("o MODE 0 VS", "w375"): 1.88, ("o MODE 2 VS", "w375"): 2.31, ("o MODE 3 VS", "w375"): 2.38,
    ("o MODE 0 splitK+reduce", "w375"): 1.94, ("o MODE 2 splitK+reduce", "w375"): 2.44, ("o MODE 3 splitK+reduce", "w375"): 2.01,
    ("k_maxpool5", "w375"): 0.0, ("k_sppf_pools", "w375"): 0.0, ("k_upsample2", "w375"): 0.0,
}
