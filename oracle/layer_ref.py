"""Float64 single-op references of the U-Net's layers and a per-element error bound.  TEST INFRASTRUCTURE.

Only ``tests/`` imports this module; nothing under ``openglottal_amd/`` does.

Every reference here is computed from the GPU's OWN input tensor of the op (``UNet.activation``), so one launch is judged in
isolation from all upstream error.  The ops are those of ``unet_oracle`` (the reference's arithmetic), in float64:

* ``conv3``  3x3 conv (pad 1, no bias) + eval BatchNorm (eps ``unet_oracle.BN_EPS``) + ReLU;
* ``first``  the same op on u8 frames scaled by 1/255 (utils.py:235);
* ``pool``   2x2 max-pool (exact: compared bit for bit);
* ``convt``  ConvTranspose 2x2 stride 2 + bias;
* ``head``   the 1x1 head + bias (the logits).

The bound of an output element is ``kappa_form * 2^-24 * M + FLOOR`` where ``M`` is a magnitude pass of the same op in float64:
``M = |s| * conv(|x|, |w|) + |s * mu| + |beta|`` with ``s`` the folded BN scale (for ``convt`` / ``head``: ``conv(|x|, |w|) + |b|``).
ReLU is 1-Lipschitz, so the bound of the pre-activation holds after it.  Where a launch fuses two ops and the boundary between
them is not stored, the next stored tensor is checked against the composed reference with the bound
``own + |s| * conv(bound_in, |w|)`` (the fused first layer at ``keep_taps`` 0, the fused head without the ``ups.N.b`` tap).

kappa per form (fixed BEFORE any GPU run; ``tests/test_layer_ref.py`` re-derives the two emulated figures on the CPU and checks
that every mutant of a kernel's arithmetic still exceeds the bound):

* ``direct`` = 16.  Direct f32 MFMA (``k_conv_mfma*``, ``k_convt_w``, ``k_conv_first``, the heads): the MFMA result is a k-ordered
  f32 fma chain; the guide's measured error against float64 is 0.75-1.5e-7 * sum|a*b| at K <= 1024 (kappa 1.3-2.5) and 3.5e-7 at
  K = 4096 (kappa 5.9); the largest K here is 512 channels x 9 taps = 4608.  The folded scale / shift (rounded once from
  float64) and the epilogue's fma add two roundings of at most |s * acc| and |shift|, both inside M.  16 = 2.7x the K = 4096 figure.
* ``wino`` = 24.  Winograd F(2x2,3x3) (``k_conv_wino*``): the transforms re-associate the sums, so the error is measured against
  the direct magnitude M, not derived.  ``wino_f32`` below emulates the kernel's arithmetic in numpy f32 (B^T d B adds in f32,
  U = G g G^T in float64 rounded once, a k-ordered f32 sum over the channels with one rounding per product and per add, A^T M A
  adds in f32, the epilogue); on the matrix's nets (random weights; random / all-0 / all-255 / 0-255 checkerboard / one-pixel
  stripe frames and their quadrant mosaic; every 3x3 layer; the seed-3 nets and the five-level net of the GPU matrix with its own
  weights and frames) the worst |err| / (2^-24 M) it reaches is 8.6 (``WINO_EMULATED_MAX``: downs.0.b of that five-level net, whose
  3-channel input from the special frames is the hardest case).  24 = 2.8x that; the weakest mutant of ``tests/test_layer_ref.py``
  (BN eps x10) is still ~20x over.  On the GPU the same layer, weights and frames reach 10.6 (0.44 of the bound): the kernel's
  packed sign-fma transforms round ~1.25x worse than the emulation's plain adds there; every other Winograd layer stays <= 3.5.
* ``split`` = 16.  Split precision (``k_conv_mfma_h``, precision 1): v = hi + lo * 2^-11 with f16 hi / lo, three exact f16
  products hi*hi + (hi*lo + lo*hi) * 2^-11 in f32 accumulation, the lo*lo term dropped, and every stored activation rounded to a
  hi / lo pair again.  ``split_f32`` emulates it; the worst emulated ratio is 3.9 (``SPLIT_EMULATED_MAX``).  16 = 4x that; the
  dropped a_lo * b_hi product (the mutant closest to the arithmetic's own error) is ~100x over.

* ``f16`` = 16.  The f16 mode (``k_conv_mfma_f``, ``k_conv_first_f``, ``k_head_f``, precision 2).  Its reference is the float64 op on
  the weights the device holds: every 3x3 conv after the first layer and every transposed conv with its weights rounded to f16
  once (round to nearest even; ``f16_weights``); first-layer, BN and head weights f32.  Inputs and weights are f16 values, so
  every product is exact in f32 and only the f32 accumulation and the f32 epilogue fma err, as in ``direct``, on the instruction
  (``v_mfma_f32_32x32x16_f16``) ``split`` passes with at 16.  Every stored activation is rounded to f16 exactly once, so the check
  is not a tolerance but a condition on bits (``check_f16``): with ``e = kappa * 2^-24 * M + FLOOR`` the stored value must lie in
  ``[RNE16(ref - e), RNE16(ref + e)]`` (rounding to nearest even is monotone); on a typical layer nine of ten positive outputs
  have a single admissible f16 value.  Subnormal f16 values are ordinary values of that interval.  The pools stay bit-exact
  (the rounded max is the max of the rounded values) and the f32 logits keep the magnitude check, from the stored (rounded)
  last activation.  Unstored boundaries: the inner bound is ``e_a`` plus half an f16 ulp of ``|ref_a| + e_a``, pushed through
  ``|s| * conv(., |w|)`` (the head's ``|w| . (.)``), the interval test on the outside.  The CPU emulation
  (``tests/f16_emulation.py``, torch f32 accumulation in two memory formats) needs kappa <= 2.5 on every stored tensor and <= 3.5
  on the head (``F16_EMULATED_MAX``); 16 = 4.6x the larger.  On the GPU (``F16_GPU_MAX``) the worst stored tensor needs 2.53 (the
  f32 first layer of the (96, 192) net; every ``k_conv_mfma_f`` tensor <= 1.58) and the head 1.94.  kappa is not a knob: a layer
  that needs more is a finding about the kernel (summation order inside the MFMA, a double rounding, a flushed subnormal).

``FLOOR`` (1e-30) only keeps exact zeros and subnormal references from dividing by zero; it is far below every M of these nets.
"""

from __future__ import annotations

import numpy as np

from .unet_oracle import BN_EPS, n_levels

U = 2.0 ** -24
FLOOR = 1e-30
KAPPA = {"direct": 16.0, "wino": 24.0, "split": 16.0, "f16": 16.0}
WINO_EMULATED_MAX = 8.6      # recorded by tests/test_layer_ref.py::test_winograd_emulation_passes_at_its_kappa (asserts <= 2x this)
SPLIT_EMULATED_MAX = 3.9     # recorded by tests/test_layer_ref.py::test_split_precision_emulation_passes_at_its_kappa


# smallest kappa the CPU emulation of the f16 mode needs (tests/test_layer_ref.py::test_f16_emulation_passes_at_its_kappa asserts
# <= 2x each): "stored" = every interval-checked tensor (first layer, 3x3 convs, transposed convs), "head" = the f32 logits
F16_EMULATED_MAX = {"stored": 2.5, "head": 3.5}
# the same two figures on the MI355X over the f16 rows of GPU_CASES and the f32 entry point (tests/test_gpu_layer_parity.py prints
# them per layer): "stored" is downs.0.a of the (96, 192) net (the f32 first-layer chain, rounded); the worst
# k_conv_mfma_f tensor is ups.1.b of the same net at 1.58, the worst transposed conv ups.6 of the full net at 1.12; "head" is the
# full-width net's.  Recorded, not asserted: the gate is KAPPA["f16"].
F16_GPU_MAX = {"stored": 2.53, "head": 1.94}


# ───────────────────────────── float64 ops ─────────────────────────────


def _t(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


def conv3_raw(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """x [B,Ci,H,W], w [Co,Ci,3,3] -> [B,Co,H,W] float64 (pad 1, cross-correlation, no bias)."""
    import torch.nn.functional as F

    return F.conv2d(_t(x), _t(w), None, 1, 1).numpy()


def fold_bn(sd: dict, bn: str, eps: float = BN_EPS):
    """Eval BatchNorm as y = s * conv + shift, float64; also the magnitude of the affine part |s * mu| + |beta|."""
    g, b = sd[bn + ".weight"].astype(np.float64), sd[bn + ".bias"].astype(np.float64)
    mu, var = sd[bn + ".running_mean"].astype(np.float64), sd[bn + ".running_var"].astype(np.float64)
    s = g / np.sqrt(var + eps)
    return s, b - mu * s, np.abs(s * mu) + np.abs(b)


def conv3_bn_relu(sd: dict, w_key: str, bn: str, x: np.ndarray, eps: float = BN_EPS):
    """(ref, pre-activation, M) of conv3x3 + BN + ReLU on x (float64)."""
    w = sd[w_key]
    s, shift, aff = fold_bn(sd, bn, eps)
    pre = s[None, :, None, None] * conv3_raw(x, w) + shift[None, :, None, None]
    M = np.abs(s)[None, :, None, None] * conv3_raw(np.abs(x), np.abs(w)) + aff[None, :, None, None]
    return np.maximum(pre, 0.0), pre, M


def first_input(gray: np.ndarray) -> np.ndarray:
    """u8 frames [B,H,W] -> the first layer's input [B,1,H,W] (utils.py:235), float64."""
    return (np.asarray(gray, dtype=np.float64) / 255.0)[:, None]


def maxpool2(x: np.ndarray) -> np.ndarray:
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).max(axis=(3, 5))


def convt_raw(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    import torch.nn.functional as F

    return F.conv_transpose2d(_t(x), _t(w), None, 2).numpy()


def convt(sd: dict, key: str, x: np.ndarray):
    """(ref, M) of ConvTranspose2d(k=2, s=2) + bias."""
    w, b = sd[key + ".weight"], sd[key + ".bias"].astype(np.float64)
    ref = convt_raw(x, w) + b[None, :, None, None]
    M = convt_raw(np.abs(x), np.abs(w)) + np.abs(b)[None, :, None, None]
    return ref, M


def head(sd: dict, x: np.ndarray):
    """(ref, M) of the 1x1 head: logits [B,1,H,W]."""
    w, b = sd["head.weight"][:, :, 0, 0].astype(np.float64), sd["head.bias"].astype(np.float64)
    ref = np.einsum("oc,bchw->bohw", w, x.astype(np.float64)) + b[None, :, None, None]
    M = np.einsum("oc,bchw->bohw", np.abs(w), np.abs(x.astype(np.float64))) + np.abs(b)[None, :, None, None]
    return ref, M


# ───────────────────────────── the check ─────────────────────────────


class LayerMismatch(AssertionError):
    pass


def check(name: str, got: np.ndarray, ref: np.ndarray, bound: np.ndarray, frames=None, tile=(16, 16)) -> float:
    """|got - ref| <= bound elementwise ([B,C,H,W]); returns the worst |err| / bound.  On failure the message names the layer, the
    frame, the channel, (y, x), the ``tile``-sized grid cell (y, x) falls in (16 x 16: the output tile of k_conv_wino<1> / <2>, two
    8 x 16 tiles of the direct kernels), the Winograd 2 x 2 output window and its position, and the worst ratio."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    if not np.all(np.isfinite(got)):
        b, c, y, x = (int(v) for v in np.argwhere(~np.isfinite(got))[0])
        raise LayerMismatch(f"{name}: non-finite value {got[b, c, y, x]} at frame {_frame(frames, b)} ch {c} (y,x)=({y},{x})")
    ratio = np.abs(got - ref) / bound
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        b, c, y, x = (int(v) for v in np.unravel_index(int(np.argmax(ratio)), ratio.shape))
        n_bad = int((ratio > 1.0).sum())
        raise LayerMismatch(
            f"{name}: |err|/bound = {worst:.3g} at frame {_frame(frames, b)} ch {c} (y,x)=({y},{x}) in {tile[0]}x{tile[1]} grid cell "
            f"({y // tile[0]},{x // tile[1]}) at ({y % tile[0]},{x % tile[1]}) inside it, Winograd 2x2 window ({y // 2},{x // 2}) pos ({y % 2},{x % 2}); got {got[b, c, y, x]!r} ref {ref[b, c, y, x]!r} "
            f"bound {bound[b, c, y, x]:.3g}; {n_bad} element(s) over the bound")
    return worst


def check_exact(name: str, got: np.ndarray, ref: np.ndarray, frames=None) -> None:
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    if len(bad):
        b, c, y, x = (int(v) for v in bad[0])
        raise LayerMismatch(f"{name}: not bit-identical at frame {_frame(frames, b)} ch {c} (y,x)=({y},{x}): got {got[b, c, y, x]!r} "
                            f"ref {ref[b, c, y, x]!r}; {len(bad)} element(s) differ")


def _frame(frames, b):
    return b if frames is None else frames[b]


def bound_of(M: np.ndarray, kappa: float) -> np.ndarray:
    return kappa * U * M + FLOOR


# ───────────────────────────── the f16 form: a condition on bits ─────────────────────────────


def rne16(v) -> np.ndarray:
    """float64 -> the nearest f16 value (ties to even, subnormals kept, one rounding), as float64."""
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=np.float64).astype(np.float16).astype(np.float64)


def half_ulp16(v) -> np.ndarray:
    """Half the f16 spacing at magnitude |v|: the most a single rounding to f16 moves a value of that magnitude."""
    v = np.abs(np.asarray(v, dtype=np.float64))
    _, ex = np.frexp(v)
    return np.where(v > 0, np.maximum(np.ldexp(1.0, ex - 12), 2.0 ** -25), 2.0 ** -25)


def f16_weights(sd: dict) -> dict:
    """The weights an f16-mode device holds: every 3x3 conv after the first layer and every transposed conv rounded to f16 once
    (ties to even); first-layer weights, BN and the head stay f32."""
    out = dict(sd)
    for k, v in sd.items():
        conv3 = k.endswith(".weight") and np.ndim(v) == 4 and ".net." in k and k != "downs.0.net.0.weight"
        convt_w = k.endswith(".weight") and np.ndim(v) == 4 and k.startswith("ups.") and ".net." not in k
        if conv3 or convt_w:
            out[k] = np.asarray(v, np.float32).astype(np.float16).astype(np.float32)
    return out


def f16_needed(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """Per element, the smallest e for which the f16 value ``got`` lies in [RNE16(ref - e), RNE16(ref + e)]: the distance from
    ``ref`` to the set of reals that round to ``got`` (0 where ``got`` is the rounded reference)."""
    g16 = np.asarray(got).astype(np.float16)
    g = g16.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        up = np.nextafter(g16, np.float16(np.inf)).astype(np.float64)
        dn = np.nextafter(g16, np.float16(-np.inf)).astype(np.float64)
        return np.maximum(0.0, np.maximum(ref - (g + up) / 2, (g + dn) / 2 - ref))


def check_f16(name: str, got: np.ndarray, ref: np.ndarray, e: np.ndarray, frames=None, tile=(16, 16), kappa: float = KAPPA["f16"]) -> float:
    """RNE16(ref - e) <= got <= RNE16(ref + e) elementwise ([B,C,H,W]); every ``got`` must be a finite f16 value.  ``e`` is the
    f32 error bound of the value BEFORE its one rounding to f16 (``bound_of(M, kappa)``, or a composed bound).  Returns the
    smallest kappa that would have admitted every element (``kappa`` scaled by the largest needed e / e).  On failure the message
    names the layer, the frame, the channel, (y, x), the ``tile``-sized grid cell, got, ref, both interval ends and the number of
    elements outside."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == e.shape, (name, got.shape, ref.shape, e.shape)
    if not np.all(np.isfinite(got)):
        b, c, y, x = (int(v) for v in np.argwhere(~np.isfinite(got))[0])
        raise LayerMismatch(f"{name}: non-finite value {got[b, c, y, x]} at frame {_frame(frames, b)} ch {c} (y,x)=({y},{x})")
    not16 = np.argwhere(rne16(got) != got)
    if len(not16):
        b, c, y, x = (int(v) for v in not16[0])
        raise LayerMismatch(f"{name}: stored value {got[b, c, y, x]!r} at frame {_frame(frames, b)} ch {c} (y,x)=({y},{x}) is not an f16 "
                            f"value; {len(not16)} such element(s)")
    lo, hi = rne16(ref - e), rne16(ref + e)
    need = f16_needed(got, ref) / e
    outside = (got < lo) | (got > hi)
    if outside.any():
        b, c, y, x = (int(v) for v in np.unravel_index(int(np.argmax(np.where(outside, need, -1.0))), need.shape))
        raise LayerMismatch(
            f"{name}: outside its f16 interval at frame {_frame(frames, b)} ch {c} (y,x)=({y},{x}) in {tile[0]}x{tile[1]} grid cell "
            f"({y // tile[0]},{x // tile[1]}) at ({y % tile[0]},{x % tile[1]}) inside it; got {got[b, c, y, x]!r} ref {ref[b, c, y, x]!r} "
            f"interval [{lo[b, c, y, x]!r}, {hi[b, c, y, x]!r}] (e {e[b, c, y, x]:.3g}, needs kappa {kappa * need[b, c, y, x]:.3g} of {kappa:g}); "
            f"{int(outside.sum())} element(s) outside the interval")
    return kappa * float(need.max()) if need.size else 0.0


# ───────────────────────────── the whole net, layer by layer ─────────────────────────────


def layer_names(L: int):
    """Tap names in chain order (the names of ``og_unet_get_activation``)."""
    out = []
    for i in range(L):
        out += [f"downs.{i}.a", f"downs.{i}.b", f"pool{i}"]
    out += ["bottleneck.a", "bottleneck.b"]
    for j in range(L):
        out += [f"ups.{2 * j}", f"ups.{2 * j + 1}.a", f"ups.{2 * j + 1}.b"]
    return out


def check_net(sd: dict, gray: np.ndarray, get, logits: np.ndarray, kappa: dict, frames=None, mask=None, area=None,
              threshold: float = 0.5, fused_first: bool = False, fused_head: bool = False, tile=(16, 16), form: str = "") -> dict:
    """Every layer tensor of one forward against its float64 reference computed from the GPU's own input.

    ``get(name)`` returns the GPU's tap ``[B,C,H,W]`` (the frames of ``gray``); ``logits`` ``[B,H,W]``; ``kappa`` maps the op kind
    (``first``, ``conv3``, ``convt``, ``head``) to the form's kappa.  ``fused_first``: ``downs.0.a`` was never stored, ``downs.0.b``
    is checked against the composed reference.  ``fused_head``: ``ups.N.b`` was never stored, the logits are checked against the
    composed reference.  ``mask`` / ``area``: checked exactly against the GPU's own logits.  Returns {layer: worst |err| / bound}.

    ``form="f16"``: the reference weights are ``f16_weights(sd)``, every stored tensor goes through ``check_f16`` (the interval
    test), the pools stay bit-exact, the f32 logits keep the magnitude check; the returned figures are then the smallest kappa
    each layer needs (for the head: its |err| / bound times its kappa).
    """
    L = n_levels(sd)
    f16 = form == "f16"
    sdw = f16_weights(sd) if f16 else sd
    worst = {}
    cache = {}

    def tap(n):
        if n not in cache:
            cache[n] = np.asarray(get(n), dtype=np.float64)
        return cache[n]

    def dc(prefix, x_in, idx):
        return conv3_bn_relu(sdw, f"{prefix}.net.{idx}.weight", f"{prefix}.net.{idx + 1}", x_in)

    def chk(name, got, ref, bound, kind):
        if f16:
            return check_f16(name, got, ref, bound, frames, tile, kappa[kind])
        return check(name, got, ref, bound, frames, tile)

    def stored(bound, ref):   # the bound of a boundary that is not stored, as the next op reads it: rounded to f16 once in the f16 form
        return bound + half_ulp16(np.abs(ref) + bound) if f16 else bound

    x0 = first_input(gray)
    for i in range(L):
        p = f"downs.{i}"
        if i == 0:
            ref_a, _, M_a = dc(p, x0, 0)
            b_a = bound_of(M_a, kappa["first"])
            if fused_first:   # downs.0.b from the frames: own bound + |s| conv(bound_a, |w|)
                ref_b, _, M_b = dc(p, ref_a, 3)
                s, _, _ = fold_bn(sd, p + ".net.4")
                bnd = bound_of(M_b, kappa["conv3"]) + np.abs(s)[None, :, None, None] * conv3_raw(stored(b_a, ref_a), np.abs(sdw[p + ".net.3.weight"]))
                worst[p + ".b (fused first)"] = chk(p + ".b (fused with the first layer)", tap(p + ".b"), ref_b, bnd, "conv3")
            else:
                worst[p + ".a"] = chk(p + ".a", tap(p + ".a"), ref_a, b_a, "first")
        else:
            ref_a, _, M_a = dc(p, tap(f"pool{i - 1}"), 0)
            worst[p + ".a"] = chk(p + ".a", tap(p + ".a"), ref_a, bound_of(M_a, kappa["conv3"]), "conv3")
        if not (i == 0 and fused_first):
            ref_b, _, M_b = dc(p, tap(p + ".a"), 3)
            worst[p + ".b"] = chk(p + ".b", tap(p + ".b"), ref_b, bound_of(M_b, kappa["conv3"]), "conv3")
        check_exact(f"pool{i}", tap(f"pool{i}"), maxpool2(tap(p + ".b")), frames)
        worst[f"pool{i}"] = 0.0
    ref, _, M = dc("bottleneck", tap(f"pool{L - 1}"), 0)
    worst["bottleneck.a"] = chk("bottleneck.a", tap("bottleneck.a"), ref, bound_of(M, kappa["conv3"]), "conv3")
    ref, _, M = dc("bottleneck", tap("bottleneck.a"), 3)
    worst["bottleneck.b"] = chk("bottleneck.b", tap("bottleneck.b"), ref, bound_of(M, kappa["conv3"]), "conv3")
    hs = kappa["head"] if f16 else 1.0      # f16 form: the head's figure in kappa units, like the other layers'
    for j in range(L):
        i = L - 1 - j
        src = "bottleneck.b" if j == 0 else f"ups.{2 * j - 1}.b"
        ref, M = convt(sdw, f"ups.{2 * j}", tap(src))
        n = f"ups.{2 * j}"
        worst[n] = chk(n, tap(n), ref, bound_of(M, kappa["convt"]), "convt")
        p = f"ups.{2 * j + 1}"
        cat = np.concatenate([tap(f"downs.{i}.b"), tap(n)], axis=1)      # skip first (unet.py:86)
        ref, _, M = dc(p, cat, 0)
        worst[p + ".a"] = chk(p + ".a", tap(p + ".a"), ref, bound_of(M, kappa["conv3"]), "conv3")
        ref_b, _, M_b = dc(p, tap(p + ".a"), 3)
        if j == L - 1 and fused_head:   # logits from ups.N.a: own bound + |w_head| . bound_b
            b_b = stored(bound_of(M_b, kappa["conv3"]), ref_b)
            ref_h, M_h = head(sd, ref_b)
            bnd = bound_of(M_h, kappa["head"]) + head_abs(sd, b_b)
            worst["head (fused)"] = hs * check("head (fused with the last conv)", logits[:, None], ref_h, bnd, frames, tile)
        else:
            worst[p + ".b"] = chk(p + ".b", tap(p + ".b"), ref_b, bound_of(M_b, kappa["conv3"]), "conv3")
    if not fused_head:
        ref_h, M_h = head(sd, tap(f"ups.{2 * L - 1}.b"))
        worst["head"] = hs * check("head", logits[:, None], ref_h, bound_of(M_h, kappa["head"]), frames, tile)
    if mask is not None:
        check_mask(logits, mask, threshold, frames)
    if area is not None:
        assert mask is not None
        exp = (np.asarray(mask) > 0).reshape(len(mask), -1).sum(1)
        assert np.array_equal(np.asarray(area), exp), ("area is not the popcount of the mask", area, exp)
    return worst


def head_abs(sd: dict, x: np.ndarray) -> np.ndarray:
    w = np.abs(sd["head.weight"][:, :, 0, 0].astype(np.float64))
    return np.einsum("oc,bchw->bohw", w, x)


def check_mask(logits: np.ndarray, mask: np.ndarray, threshold: float, frames=None, band: float = 2.0 ** -22) -> int:
    """mask > 0 must equal logit > logit(threshold) -- on the GPU's own logits, bit for bit -- except within ``band`` of the
    threshold logit, where the kernels' f32 sigmoid (1 / (1 + expf(-v)) > thr, the reference's rule) rounds to thr itself
    (at thr 0.5: any 0 < v < 2^-25 gives exactly 0.5).  Returns the number of pixels inside the band."""
    lg = np.asarray(logits, dtype=np.float64)
    t = float(np.log(threshold / (1.0 - threshold)))
    want = lg > t
    near = np.abs(lg - t) <= band * max(1.0, abs(t))
    bad = np.argwhere(((np.asarray(mask) > 0) != want) & ~near)
    if len(bad):
        b, y, x = (int(v) for v in bad[0])
        raise LayerMismatch(f"mask: frame {_frame(frames, b)} (y,x)=({y},{x}) mask {int(mask[b, y, x])} logit {lg[b, y, x]!r} "
                            f"threshold logit {t!r}; {len(bad)} pixel(s) differ")
    return int(near.sum())


# ───────────────────────────── f32 emulations of the kernel forms (κ derivation) ─────────────────────────────

_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], dtype=np.float64)
_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _bt_axis(d, axis):
    """B^T along one axis of a [..4..] f32 array, one f32 rounding per add / subtract (the kernels' x[ia] +- x[ib])."""
    t = np.moveaxis(d, axis, 0)
    out = np.stack([t[0] - t[2], t[1] + t[2], t[2] - t[1], t[1] - t[3]])
    return np.moveaxis(out.astype(np.float32), 0, axis)


def _at_axis(m, axis):
    t = np.moveaxis(m, axis, 0)
    out = np.stack([(t[0] + t[1]) + t[2], (t[1] - t[2]) - t[3]])
    return np.moveaxis(out.astype(np.float32), 0, axis)


def wino_transform_weights(w: np.ndarray) -> np.ndarray:
    """U = G g G^T per (co, ci), float64, rounded once to f32 (as the host packs it): [Co,Ci,4,4]."""
    return _f32(np.einsum("ij,ocjk,lk->ocil", _G, w.astype(np.float64), _G))


def wino_f32(x: np.ndarray, w: np.ndarray, s: np.ndarray, shift: np.ndarray, relu: bool = True, U_w=None) -> np.ndarray:
    """numpy f32 emulation of a k_conv_wino* launch: conv3x3 (pad 1) via F(2x2,3x3) + the fma epilogue (+ ReLU).
    x [B,Ci,H,W] f32, w [Co,Ci,3,3]."""
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    th, tw = (H + 1) // 2, (W + 1) // 2                               # odd maps: the last window row / column reads padding
    xp = np.zeros((B, Ci, 2 * th + 2, 2 * tw + 2), np.float32)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    d = np.empty((B, Ci, th, tw, 4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            d[..., i, j] = xp[:, :, i:i + 2 * th:2, j:j + 2 * tw:2]
    V = _bt_axis(_bt_axis(d, 4), 5)                                   # [B,Ci,th,tw,4,4]
    Uw = wino_transform_weights(w) if U_w is None else U_w            # [Co,Ci,4,4]
    acc = np.zeros((B, Co, th, tw, 4, 4), np.float32)
    for c in range(Ci):                                               # k-ordered f32 sum over the channels
        prod = (Uw[None, :, c, None, None] * V[:, c, None]).astype(np.float32)
        acc = (acc + prod).astype(np.float32)
    Y = _at_axis(_at_axis(acc, 4), 5)                                 # [B,Co,th,tw,2,2]
    y = Y.transpose(0, 1, 2, 4, 3, 5).reshape(B, Co, 2 * th, 2 * tw)[:, :, :H, :W]
    out = (y * _f32(s)[None, :, None, None] + _f32(shift)[None, :, None, None]).astype(np.float32)
    return np.maximum(out, 0).astype(np.float32) if relu else out


def split_hilo(v: np.ndarray):
    """v -> (hi, lo) f16 with v ~ hi + lo * 2^-11 (the kernels' split)."""
    v = _f32(v)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def join_hilo(hi, lo) -> np.ndarray:
    return (hi.astype(np.float32) + lo.astype(np.float32) * np.float32(1.0 / 2048.0)).astype(np.float32)


def split_f32(x: np.ndarray, w: np.ndarray, s: np.ndarray, shift: np.ndarray, relu: bool = True, drop: str = "") -> np.ndarray:
    """numpy emulation of a k_conv_mfma_h launch: x (a decoded hi / lo activation) and w split into f16 hi / lo, three products
    (hi*hi, hi*lo, lo*hi; lo*lo dropped) summed in f32 per tap, the two correction products scaled by 2^-11 at the end, the fma
    epilogue and the store as a hi / lo pair.  ``drop="a_lo_b_hi"`` omits the x_lo * w_hi product (a mutant)."""
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    xh, xl = split_hilo(x)
    wh, wl = split_hilo(w)
    xp_h = np.zeros((B, Ci, H + 2, W + 2), np.float32)
    xp_l = np.zeros_like(xp_h)
    xp_h[:, :, 1:-1, 1:-1] = xh.astype(np.float32)
    xp_l[:, :, 1:-1, 1:-1] = xl.astype(np.float32)
    acc = np.zeros((B, Co, H, W), np.float32)
    cor = np.zeros((B, Co, H, W), np.float32)
    whf, wlf = wh.astype(np.float32), wl.astype(np.float32)
    for dy in range(3):
        for dx in range(3):
            ah = xp_h[:, :, dy:dy + H, dx:dx + W]
            al = xp_l[:, :, dy:dy + H, dx:dx + W]
            # f16 x f16 products are exact in f32; the sum over the channels in f32
            acc = (acc + np.einsum("oc,bchw->bohw", whf[:, :, dy, dx], ah, dtype=np.float32)).astype(np.float32)
            c = np.einsum("oc,bchw->bohw", wlf[:, :, dy, dx], ah, dtype=np.float32)
            if drop != "a_lo_b_hi":
                c = (c + np.einsum("oc,bchw->bohw", whf[:, :, dy, dx], al, dtype=np.float32)).astype(np.float32)
            cor = (cor + c).astype(np.float32)
    acc = (acc + cor * np.float32(1.0 / 2048.0)).astype(np.float32)
    out = (acc * _f32(s)[None, :, None, None] + _f32(shift)[None, :, None, None]).astype(np.float32)
    if relu:
        out = np.maximum(out, 0).astype(np.float32)
    return join_hilo(*split_hilo(out))


# ───────────────────────────── special frames ─────────────────────────────


def special_frames(H: int, W: int, seed: int = 0) -> dict:
    """The frames every GPU case reads back: a quadrant mosaic of the four patterns (and their seams), random noise, all-0, all-255,
    the 0/255 checkerboard (the worst case for the Winograd transforms' cancellation) and one-pixel stripes."""
    yy, xx = np.mgrid[0:H, 0:W]
    checker = (((yy + xx) & 1) * 255).astype(np.uint8)
    stripes = ((xx & 1) * 255).astype(np.uint8)
    zeros = np.zeros((H, W), np.uint8)
    full = np.full((H, W), 255, np.uint8)
    mosaic = zeros.copy()
    h2, w2 = H // 2, W // 2
    mosaic[:h2, w2:] = 255
    mosaic[h2:, :w2] = checker[h2:, :w2]
    mosaic[h2:, w2:] = ((yy[h2:, w2:] & 1) * 255).astype(np.uint8)     # horizontal stripes in the last quadrant
    rnd = np.random.RandomState(seed).randint(0, 256, (H, W), dtype=np.uint8)
    return {"mosaic": mosaic, "random": rnd, "zeros": zeros, "full": full, "checker": checker, "stripes": stripes}


# ───────────────────────────── the GPU matrix (tests/test_gpu_layer_parity.py; its coverage is checked on the CPU) ─────────────────────────────

FULL = (32, 64, 128, 256)


# Every instantiation the U-Net chain can launch at precision 0 and 1, by a short label -> (its text in og_unet_plan as
# ``plan_instantiations`` reads it, its label in UNet.profile (None: it runs inside the launch before it), a smallest net / frame
# shape / micro-batch / option set that reaches it: an edge shape wherever the planner allows one).  tests/test_layer_ref.py closes
# the list on the CPU: an option sweep finds no instantiation outside it, every entry is reached by its own option set, and the
# non-f16 rows of GPU_CASES together with F32_ENTRY_CASES run every one of them, on shapes with edges wherever one can be chosen.
F32_KERNELS = {
    "convt_w": ("k_convt_w", "k_convt_w<1,1,8>", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1")),
    "epilogue<1,0,8>": ("k_splitk_epilogue<1, 0, 8>", None, ((33, 66), 32, 64, 8, "keep_taps=1,wino=0,splitk=1,splitk_fused=0")),
    "epilogue<2,0,8>": ("k_splitk_epilogue<2, 0, 8>", None, ((33, 66), 32, 64, 8, "keep_taps=1,wino=0,splitk=1,splitk_fused=0")),
    "epilogue<2,1,8>": ("k_splitk_epilogue<2, 1, 8>", None, ((33, 66), 32, 64, 8, "keep_taps=1,wino=0,splitk=1,splitk_fused=0")),
    "first<f32,split>": ("k_conv_first<float, true>", "k_conv_first<f32>", ((33, 66), 64, 64, 6, "keep_taps=1,precision=1,entry_f32=1")),
    "first<f32>": ("k_conv_first<float>", "k_conv_first<f32>", ((33, 66), 64, 64, 6, "keep_taps=1,precision=0,entry_f32=1")),
    "first<u8,split>": ("k_conv_first<uint8_t, true>", "k_conv_first<u8>", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1,precision=1")),
    "first<u8>": ("k_conv_first<uint8_t>", "k_conv_first<u8>", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1")),
    "h<1,0,16,2>": ("k_conv_mfma_h<1, 0, 16, 2, false, false>", "k_conv_mfma_h<1,0,16>", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1,precision=1")),
    "h<1,0,8,3,FIRST>": ("k_conv_mfma_h<1, 0, 8, 3, true>", "k_conv_mfma_h<1,0,8,FIRST>", ((32, 64), 96, 160, 16, "keep_taps=0,precision=1")),
    "h<1,0,8,3>": ("k_conv_mfma_h<1, 0, 8, 3, false, false>", "k_conv_mfma_h<1,0,8>", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1,precision=1")),
    "h<1,0,8,3>+splitK": ("k_conv_mfma_h<1, 0, 8, 3, false, false>+splitK", "k_conv_mfma_h<1,0,8>", ((32, 64), 96, 160, 1, "keep_taps=1,precision=1,splitk=1")),
    "h<2,0,16,2,SQ>": ("k_conv_mfma_h<2, 0, 16, 2, false, true>", "k_conv_mfma_h<2,0,16>", ((33, 66), 32, 64, 4, "keep_taps=1,precision=1")),
    "h<2,0,16,2>": ("k_conv_mfma_h<2, 0, 16, 2, false, false>", "k_conv_mfma_h<2,0,16>", ((32, 64), 96, 160, 4, "keep_taps=1,precision=1,h_square=0")),
    "h<2,0,8,3>": ("k_conv_mfma_h<2, 0, 8, 3, false, false>", "k_conv_mfma_h<2,0,8>", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1,precision=1")),
    "h<2,0,8,3>+splitK": ("k_conv_mfma_h<2, 0, 8, 3, false, false>+splitK", "k_conv_mfma_h<2,0,8>", ((32, 64), 96, 160, 1, "keep_taps=1,precision=1,splitk=1")),
    "h<2,1,8,3>": ("k_conv_mfma_h<2, 1, 8, 3, false, false>", "k_conv_mfma_h<2,1,8>", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1,precision=1")),
    "h<2,1,8,3>+splitK": ("k_conv_mfma_h<2, 1, 8, 3, false, false>+splitK", "k_conv_mfma_h<2,1,8>", ((32, 64), 96, 160, 1, "keep_taps=1,precision=1,splitk=1")),
    "head": ("k_head<false>", "k_head", ((33, 66), 32, 64, 1, "keep_taps=1,wino=0,splitk=1,splitk_nt1=0")),
    "head<split>": ("k_head<true>", "k_head", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1,precision=1")),
    "mfma<1,0,8>": ("k_conv_mfma<1, 0, 8>", "k_conv_mfma<1,0,8>", ((32, 64), 96, 160, 4, "keep_taps=1,wino=0,conv_impl=0")),
    "mfma<2,0,8>": ("k_conv_mfma<2, 0, 8>", "k_conv_mfma<2,0,8>", ((32, 64), 96, 160, 4, "keep_taps=1,wino=0,conv_impl=0")),
    "mfma<2,1,8>": ("k_conv_mfma<2, 1, 8>", "k_conv_mfma<2,1,8>", ((32, 64), 96, 160, 4, "keep_taps=1,wino=0,conv_impl=0")),
    "o<1,0,16,2>": ("k_conv_mfma_o<1, 0, 16, 2, false, false>", "k_conv_mfma_o<1,0,16>", ((33, 66), 32, 64, 64, "keep_taps=1,wino=0,tile_h=16")),
    "o<1,0,8,3,FIRST>": ("k_conv_mfma_o<1, 0, 8, 3, true>", "k_conv_mfma_o<1,0,8,FIRST>", ((32, 64), 96, 160, 16, "keep_taps=0,wino=0")),
    "o<1,0,8,3>": ("k_conv_mfma_o<1, 0, 8, 3, false, false>", "k_conv_mfma_o<1,0,8>", ((33, 66), 32, 64, 64, "keep_taps=1,wino=0,tile_h=16")),
    "o<1,0,8,3>+splitK": ("k_conv_mfma_o<1, 0, 8, 3, false, false>+splitK", "k_conv_mfma_o<1,0,8>+splitK", ((33, 66), 32, 64, 8, "keep_taps=1,wino=0,splitk=1,splitk_fused=0")),
    "o<1,0,8,3>+splitK+reduce": ("k_conv_mfma_o<1, 0, 8, 3, false, false>+splitK+reduce", "k_conv_mfma_o<1,0,8>+splitK", ((33, 66), 32, 64, 1, "keep_taps=1,wino=0,splitk=1,splitk_nt1=0")),
    "o<1,0,8,4>": ("k_conv_mfma_o<1, 0, 8, 4, false, false>", "k_conv_mfma_o<1,0,8>", ((32, 64), 96, 160, 16, "keep_taps=1,wino=0,conv_impl=3")),
    "o<2,0,16,2>": ("k_conv_mfma_o<2, 0, 16, 2, false, false>", "k_conv_mfma_o<2,0,16>", ((33, 66), 32, 64, 64, "keep_taps=1,wino=0,tile_h=16")),
    "o<2,0,8,3>": ("k_conv_mfma_o<2, 0, 8, 3, false, false>", "k_conv_mfma_o<2,0,8>", ((32, 64), 96, 160, 16, "keep_taps=1")),
    "o<2,0,8,3>+splitK": ("k_conv_mfma_o<2, 0, 8, 3, false, false>+splitK", "k_conv_mfma_o<2,0,8>+splitK", ((33, 66), 32, 64, 8, "keep_taps=1,wino=0,splitk=1,splitk_fused=0")),
    "o<2,0,8,3>+splitK+reduce": ("k_conv_mfma_o<2, 0, 8, 3, false, false>+splitK+reduce", "k_conv_mfma_o<2,0,8>+splitK", ((33, 66), 32, 64, 1, "keep_taps=1,wino=0,splitk=1,splitk_nt1=0")),
    "o<2,0,8,4>": ("k_conv_mfma_o<2, 0, 8, 4, false, false>", "k_conv_mfma_o<2,0,8>", ((32, 64), 96, 160, 16, "keep_taps=1,wino=0,conv_impl=3")),
    "o<2,1,8,3>": ("k_conv_mfma_o<2, 1, 8, 3, false, false>", "k_conv_mfma_o<2,1,8>", ((40, 80), 64, 64, 8, "keep_taps=1")),
    "o<2,1,8,3>+splitK": ("k_conv_mfma_o<2, 1, 8, 3, false, false>+splitK", "k_conv_mfma_o<2,1,8>+splitK", ((33, 66), 32, 64, 8, "keep_taps=1,wino=0,splitk=1,splitk_fused=0")),
    "o<2,1,8,3>+splitK+reduce": ("k_conv_mfma_o<2, 1, 8, 3, false, false>+splitK+reduce", "k_conv_mfma_o<2,1,8>+splitK", ((33, 66), 32, 64, 1, "keep_taps=1,wino=0,splitk=1,splitk_nt1=0")),
    "p<1,0,16,3>": ("k_conv_mfma_p<1, 0, 16, 3>", "k_conv_mfma_p<1,0,16,3>", ((32, 64), 96, 160, 4, "keep_taps=1,wino=0,conv_impl=1,tile_h=16")),
    "p<1,0,16,9>": ("k_conv_mfma_p<1, 0, 16, 9>", "k_conv_mfma_p<1,0,16,9>", ((32, 64), 96, 160, 4, "keep_taps=1,wino=0,conv_impl=1,tile_h=16,tps_nt1=9,tps_nt2=3")),
    "p<1,0,8,1>": ("k_conv_mfma_p<1, 0, 8, 1>", "k_conv_mfma_p<1,0,8,1>", ((33, 66), 32, 64, 4, "keep_taps=1,wino=0,conv_impl=1,tps_nt1=1")),
    "p<1,0,8,1>+splitK": ("k_conv_mfma_p<1, 0, 8, 1>+splitK", "k_conv_mfma_p<1,0,8,1>", ((33, 66), 32, 64, 2, "keep_taps=1,wino=0,conv_impl=1,splitk=1,tps_nt1=1")),
    "p<1,0,8,3>": ("k_conv_mfma_p<1, 0, 8, 3>", "k_conv_mfma_p<1,0,8,3>", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1")),
    "p<1,0,8,3>+splitK": ("k_conv_mfma_p<1, 0, 8, 3>+splitK", "k_conv_mfma_p<1,0,8,3>", ((32, 64), 96, 160, 1, "keep_taps=1,wino=0,conv_impl=1,splitk=1")),
    "p<1,0,8,9>": ("k_conv_mfma_p<1, 0, 8, 9>", "k_conv_mfma_p<1,0,8,9>", ((33, 66), 32, 64, 4, "keep_taps=1,wino=0,conv_impl=1,tps_nt1=9,tps_nt2=3")),
    "p<1,0,8,9>+splitK": ("k_conv_mfma_p<1, 0, 8, 9>+splitK", "k_conv_mfma_p<1,0,8,9>", ((33, 66), 32, 64, 2, "keep_taps=1,wino=0,conv_impl=1,splitk=1,tps_nt1=9,tps_nt2=3")),
    "p<2,0,16,1>": ("k_conv_mfma_p<2, 0, 16, 1>", "k_conv_mfma_p<2,0,16,1>", ((32, 64), 96, 160, 4, "keep_taps=1,wino=0,conv_impl=1,tile_h=16")),
    "p<2,0,16,3>": ("k_conv_mfma_p<2, 0, 16, 3>", "k_conv_mfma_p<2,0,16,3>", ((32, 64), 96, 160, 4, "keep_taps=1,wino=0,conv_impl=1,tile_h=16,tps_nt1=9,tps_nt2=3")),
    "p<2,0,8,1>": ("k_conv_mfma_p<2, 0, 8, 1>", "k_conv_mfma_p<2,0,8,1>", ((4, 8, 16, 32), 16, 16, 4, "keep_taps=1")),
    "p<2,0,8,1>+splitK": ("k_conv_mfma_p<2, 0, 8, 1>+splitK", "k_conv_mfma_p<2,0,8,1>", ((32, 64), 96, 160, 1, "keep_taps=1,wino=0,conv_impl=1,splitk=1")),
    "p<2,0,8,3>": ("k_conv_mfma_p<2, 0, 8, 3>", "k_conv_mfma_p<2,0,8,3>", ((33, 66), 32, 64, 4, "keep_taps=1,wino=0,conv_impl=1,tps_nt1=9,tps_nt2=3")),
    "p<2,0,8,3>+splitK": ("k_conv_mfma_p<2, 0, 8, 3>+splitK", "k_conv_mfma_p<2,0,8,3>", ((33, 66), 32, 64, 2, "keep_taps=1,wino=0,conv_impl=1,splitk=1,tps_nt1=9,tps_nt2=3")),
    "p<2,1,8,1>": ("k_conv_mfma_p<2, 1, 8, 1>", "k_conv_mfma_p<2,1,8,1>", ((33, 66), 32, 64, 4, "keep_taps=1,wino=0,conv_impl=1,tps_nt1=9,tps_nt2=3")),
    "p<2,1,8,1>+splitK": ("k_conv_mfma_p<2, 1, 8, 1>+splitK", "k_conv_mfma_p<2,1,8,1>", ((32, 64), 96, 160, 1, "keep_taps=1,wino=0,conv_impl=1,splitk=1")),
    "ps<1,1>": ("k_conv_wino_ps<1, 1>", "k_conv_wino_ps<1,1>", ((32, 64), 64, 64, 1, "keep_taps=1,wino_w=0,wino_ps=4")),
    "ps<1,2>": ("k_conv_wino_ps<1, 2>", "k_conv_wino_ps<1,2>", ((32, 64), 64, 64, 1, "keep_taps=1,wino_w=0,wino_ps=3")),
    "ps<1,4>": ("k_conv_wino_ps<1, 4>", "k_conv_wino_ps<1,4>", ((32, 64), 64, 64, 1, "keep_taps=1,wino_w=0,wino_ps=2")),
    "ps<2,1>": ("k_conv_wino_ps<2, 1>", "k_conv_wino_ps<2,1>", ((32, 64), 64, 64, 1, "keep_taps=1,wino_w=0,wino_ps=4")),
    "ps<2,2>": ("k_conv_wino_ps<2, 2>", "k_conv_wino_ps<2,2>", ((32, 64), 64, 64, 1, "keep_taps=1,wino_w=0,wino_ps=3")),
    "ps<2,4>": ("k_conv_wino_ps<2, 4>", "k_conv_wino_ps<2,4>", ((32, 64), 64, 64, 1, "keep_taps=1,wino_w=0,wino_ps=2")),
    "w<1> nt=1": ("k_conv_wino_w<1> nt=1", "k_conv_wino_w<1,1>", ((3, 6, 12, 24, 48), 64, 96, 4, "keep_taps=1")),
    "w<1> nt=2": ("k_conv_wino_w<1> nt=2", "k_conv_wino_w<2,1>", ((33, 66), 32, 64, 4, "keep_taps=1")),
    "w<2> nt=1": ("k_conv_wino_w<2> nt=1", "k_conv_wino_w<1,2>", ((32, 64), 64, 64, 1, "keep_taps=1,wino_w=3")),
    "w<2> nt=2": ("k_conv_wino_w<2> nt=2", "k_conv_wino_w<2,2>", ((32, 64), 64, 64, 1, "keep_taps=1,wino_w=3")),
    "wino<1>": ("k_conv_wino<1>", "k_conv_wino<1>", ((32, 64), 96, 160, 16, "keep_taps=1")),
    "wino<2>": ("k_conv_wino<2>", "k_conv_wino<2>", ((32, 64), 96, 160, 16, "keep_taps=1")),
    "wp nt=1": ("k_conv_wino_wp nt=1", "k_conv_wino_wp<1>", ((3, 6, 12, 24, 48), 64, 96, 4, "keep_taps=1")),
    "wp nt=2": ("k_conv_wino_wp nt=2", "k_conv_wino_wp<2>", ((33, 66), 32, 64, 1, "keep_taps=1")),
}

# instantiations the planner chooses at the full-width net on 256 x 256 only -> the rule in og_api.hip that excludes them elsewhere
EDGE_EXEMPT = {}


def is_edge_case(case) -> bool:
    """A row whose tiles have borders, whose channels are padded or whose maps are small: anything but the full-width net at 256 x 256."""
    return not (tuple(case["feats"]) == FULL and case["H"] == 256 and case["W"] == 256)


def _case(cid, feats, H, W, B, options=None, families=(), form="wino", nread=2, fused_first=False, fused_head=False, prof=(), kernels=()):
    opts = {"keep_taps": 1}
    opts.update(options or {})
    if not prof:   # every kernel family of the plan check is asserted through UNet.profile as well
        prof = [f for f in families if f.startswith("k_") and f not in ("k_splitk_epilogue", "k_sum_counts")]
    # kernels (non-f16 rows): the row's plan by instantiation, EXACTLY (F32_KERNELS labels); prof_inst: their UNet.profile labels
    prof_inst = sorted({F32_KERNELS[k][1] for k in kernels} - {None})
    return dict(id=cid, feats=tuple(feats), H=H, W=W, B=B, options=opts, families=tuple(families), form=form, nread=min(nread, B),
                fused_first=fused_first, fused_head=fused_head, prof=tuple(prof), kernels=tuple(kernels), prof_inst=tuple(prof_inst))


# families: what og_unet_plan must list for the case (``plan_families``); prof: what UNet.profile must list (``profile_families``)
GPU_CASES = [
    _case("default-64", FULL, 256, 256, 64, {}, ["k_conv_wino", "k_conv_mfma_o"], prof=["k_conv_wino", "k_conv_mfma_o"],
          kernels=["first<u8>", "o<2,1,8,3>", "wino<1>", "wino<2>"]),
    _case("default-1", FULL, 256, 256, 1, {}, ["k_conv_wino_w", "k_conv_wino_wp", "k_convt_w"], nread=1,
          prof=["k_conv_wino_w", "k_conv_wino_wp", "k_convt_w"],
          kernels=["convt_w", "first<u8>", "o<2,1,8,3>", "w<1> nt=2", "w<2> nt=1", "wp nt=2"]),
    _case("position-split-1", FULL, 256, 256, 1, {"wino_w": 0}, ["k_conv_wino_ps"], nread=1, prof=["k_conv_wino_ps"],
          kernels=["convt_w", "first<u8>", "o<2,1,8,3>", "ps<2,1>", "ps<2,2>", "ps<2,4>", "wino<1>"]),
    _case("direct-64", FULL, 256, 256, 64, {"wino": 0}, ["k_conv_mfma_o"], form="direct", prof=["k_conv_mfma_o"],
          kernels=["first<u8>", "o<1,0,8,3>", "o<2,0,16,2>", "o<2,0,8,3>", "o<2,1,8,3>"]),
    _case("direct-impl0-2", FULL, 256, 256, 2, {"wino": 0, "conv_impl": 0}, ["k_conv_mfma", "k_head"], form="direct",
          prof=["k_conv_mfma", "k_head"],
          kernels=["first<u8>", "head", "mfma<1,0,8>", "mfma<2,0,8>", "mfma<2,1,8>"]),
    _case("direct-impl1-2", FULL, 256, 256, 2, {"wino": 0, "conv_impl": 1}, ["k_conv_mfma_p"], form="direct", prof=["k_conv_mfma_p"],
          kernels=["first<u8>", "p<1,0,8,3>", "p<2,0,8,1>", "p<2,1,8,1>"]),
    _case("splitk-fused-1", FULL, 256, 256, 1, {"wino": 0, "splitk": 1}, ["k_conv_mfma_o", "splitk-parts", "splitk-fused-reduce"], form="direct", nread=1,
          prof=["splitK"],
          kernels=["first<u8>", "o<1,0,8,3>", "o<1,0,8,3>+splitK+reduce", "o<2,0,8,3>+splitK+reduce", "o<2,1,8,3>", "o<2,1,8,3>+splitK+reduce"]),
    _case("splitk-fused-2", FULL, 256, 256, 2, {"wino": 0, "splitk": 1}, ["k_conv_mfma_o", "splitk-parts", "splitk-fused-reduce"], form="direct",
          prof=["splitK"],
          kernels=["first<u8>", "o<1,0,8,3>", "o<1,0,8,3>+splitK+reduce", "o<2,0,8,3>", "o<2,0,8,3>+splitK+reduce", "o<2,1,8,3>", "o<2,1,8,3>+splitK+reduce"]),
    _case("splitk-epilogue-2", FULL, 256, 256, 2, {"wino": 0, "splitk": 1, "splitk_fused": 0}, ["splitk-parts", "k_splitk_epilogue"], form="direct",
          prof=["splitK"],
          kernels=["epilogue<1,0,8>", "epilogue<2,0,8>", "epilogue<2,1,8>", "first<u8>", "o<1,0,8,3>", "o<1,0,8,3>+splitK", "o<2,0,8,3>", "o<2,0,8,3>+splitK", "o<2,1,8,3>", "o<2,1,8,3>+splitK"]),
    _case("splitk-nt1-0-steps9-1", FULL, 256, 256, 1, {"wino": 0, "splitk": 1, "splitk_nt1": 0, "splitk_min_steps": 9},
          ["splitk-parts", "splitk-fused-reduce"], form="direct", nread=1, prof=["splitK"],
          kernels=["first<u8>", "o<1,0,8,3>", "o<2,0,8,3>+splitK+reduce", "o<2,1,8,3>", "o<2,1,8,3>+splitK+reduce", "p<2,0,8,1>"]),
    _case("split-precision-64", FULL, 256, 256, 64, {"precision": 1}, ["k_conv_mfma_h"], form="split", prof=["k_conv_mfma_h"],
          kernels=["first<u8,split>", "h<1,0,16,2>", "h<2,0,16,2,SQ>", "h<2,1,8,3>", "head<split>"]),
    _case("split-precision-1", FULL, 256, 256, 1, {"precision": 1}, ["k_conv_mfma_h"], form="split", nread=1, prof=["k_conv_mfma_h"],
          kernels=["first<u8,split>", "h<1,0,16,2>", "h<2,0,16,2,SQ>", "h<2,1,8,3>", "head<split>"]),
    _case("split-precision-splitk-1", FULL, 256, 256, 1, {"precision": 1, "splitk": 1}, ["k_conv_mfma_h", "splitk-parts"],
          form="split", nread=1, prof=["k_conv_mfma_h"],
          kernels=["first<u8,split>", "h<1,0,16,2>", "h<2,0,16,2,SQ>", "h<2,0,8,3>+splitK", "h<2,1,8,3>", "h<2,1,8,3>+splitK", "head<split>"]),
    _case("fused-first-and-head-64", FULL, 256, 256, 64, {"wino": 0, "keep_taps": 0}, ["first-fused", "k_sum_counts"], form="direct",
          fused_first=True, fused_head=True, prof=["first-fused"],
          kernels=["o<1,0,8,3,FIRST>", "o<1,0,8,3>", "o<2,0,16,2>", "o<2,0,8,3>", "o<2,1,8,3>"]),
    _case("fused-head-wino-64", FULL, 256, 256, 64, {"keep_taps": 0}, ["k_conv_wino", "k_sum_counts"], fused_head=True,
          prof=["k_conv_wino"],
          kernels=["first<u8>", "o<2,1,8,3>", "wino<1>", "wino<2>"]),
    _case("unfused-head-2", FULL, 256, 256, 2, {"fuse_head": 0}, ["k_head"], prof=["k_head"],
          kernels=["convt_w", "first<u8>", "head", "o<2,1,8,3>", "w<1> nt=2", "w<2> nt=2", "wino<1>", "wp nt=2"]),
    _case("tiles-128x256", (32, 64), 128, 256, 64, {}, ["k_conv_wino"], prof=["k_conv_wino"],
          kernels=["first<u8>", "o<2,1,8,3>", "wino<1>", "wino<2>"]),
    _case("tiles-96x160", (32, 64), 96, 160, 16, {}, ["k_conv_wino"], nread=4, prof=["k_conv_wino"],
          kernels=["first<u8>", "o<2,0,8,3>", "o<2,1,8,3>", "wino<1>", "wino<2>"]),
    _case("tiles-96x160-direct", (32, 64), 96, 160, 16, {"wino": 0}, ["k_conv_mfma_o"], form="direct", nread=4,
          kernels=["first<u8>", "o<1,0,8,3>", "o<2,0,8,3>", "o<2,1,8,3>"]),
    _case("padded-40x80-64x64", (40, 80), 64, 64, 8, {}, ["k_conv_wino_w", "k_head"], nread=6,
          kernels=["convt_w", "first<u8>", "head", "o<2,1,8,3>", "p<1,0,8,3>", "w<1> nt=1", "w<2> nt=2"]),
    _case("padded-33x66-32x64", (33, 66), 32, 64, 4, {}, ["k_conv_wino_w", "k_conv_mfma_p", "k_head"], nread=4,
          kernels=["convt_w", "first<u8>", "head", "p<1,0,8,3>", "w<1> nt=2"]),
    _case("padded-33x66-32x64-direct", (33, 66), 32, 64, 4, {"wino": 0}, ["k_conv_mfma_p"], form="direct", nread=4,
          kernels=["convt_w", "first<u8>", "head", "p<1,0,8,3>", "p<2,0,8,1>"]),
    _case("bottleneck-1x1-16x16", (4, 8, 16, 32), 16, 16, 4, {}, ["k_conv_mfma_p", "k_convt_w"], nread=4,
          kernels=["convt_w", "first<u8>", "p<1,0,8,3>", "p<2,0,8,1>"]),
    _case("maps-1x16-16x256", (4, 8, 16, 32), 16, 256, 2, {}, ["k_conv_mfma_p"], nread=2,
          kernels=["convt_w", "first<u8>", "p<1,0,8,3>", "p<2,0,8,1>"]),
    _case("five-levels-64x96", (3, 6, 12, 24, 48), 64, 96, 4, {}, ["k_conv_wino_w", "k_conv_wino_wp", "k_conv_mfma_p"], nread=4,
          kernels=["convt_w", "first<u8>", "p<1,0,8,3>", "p<2,0,8,1>", "w<1> nt=1", "wp nt=1"]),
    _case("large-512x512", (32, 64), 512, 512, 8, {}, ["k_conv_wino"], nread=1,
          kernels=["first<u8>", "o<2,1,8,3>", "wino<1>", "wino<2>"]),
    # every remaining instantiation of the f32 chains (F32_KERNELS), on the smallest shapes that still have edges.  Ten of these
    # rows (REDUNDANT_FOR_COVERAGE below) are the only cover of no instantiation: they judge kernels other rows run on a second
    # shape (padded K, 1 x 1 maps, five levels, partial tiles, forced PN), so dropping one of them fails no coverage test.
    _case("persistent-tps9-33x66", (33, 66), 32, 64, 4, {"wino": 0, "conv_impl": 1, "tps_nt1": 9, "tps_nt2": 3}, form="direct", nread=4,
          kernels=["first<u8>", "head", "p<1,0,8,9>", "p<2,0,8,3>", "p<2,1,8,1>"]),
    _case("persistent-tps1-33x66", (33, 66), 32, 64, 4, {"wino": 0, "conv_impl": 1, "tps_nt1": 1}, form="direct", nread=4,
          kernels=["first<u8>", "head", "p<1,0,8,1>", "p<2,0,8,1>", "p<2,1,8,1>"]),
    _case("persistent-tile16-96x160", (32, 64), 96, 160, 4, {"wino": 0, "conv_impl": 1, "tile_h": 16}, form="direct", nread=4,
          kernels=["first<u8>", "p<1,0,16,3>", "p<1,0,8,3>", "p<2,0,16,1>", "p<2,0,8,1>", "p<2,1,8,1>"]),
    _case("persistent-tile16-tps9-96x160", (32, 64), 96, 160, 4, {"wino": 0, "conv_impl": 1, "tile_h": 16, "tps_nt1": 9, "tps_nt2": 3}, form="direct", nread=4,
          kernels=["first<u8>", "p<1,0,16,9>", "p<1,0,8,9>", "p<2,0,16,3>", "p<2,0,8,3>", "p<2,1,8,1>"]),
    _case("occupancy-tile16-33x66-64", (33, 66), 32, 64, 64, {"wino": 0, "tile_h": 16}, form="direct", nread=4,
          kernels=["first<u8>", "head", "o<1,0,16,2>", "o<1,0,8,3>", "o<2,0,16,2>", "o<2,1,8,3>"]),
    _case("occupancy-occ4-96x160", (32, 64), 96, 160, 16, {"wino": 0, "conv_impl": 3}, form="direct", nread=4,
          kernels=["first<u8>", "o<1,0,8,4>", "o<2,0,8,4>", "o<2,1,8,3>"]),
    _case("position-split-pn4-64x64", (32, 64), 64, 64, 1, {"wino_w": 0, "wino_ps": 2}, form="wino", nread=1,
          kernels=["convt_w", "first<u8>", "ps<1,4>", "ps<2,4>"]),
    _case("position-split-pn2-64x64", (32, 64), 64, 64, 1, {"wino_w": 0, "wino_ps": 3}, form="wino", nread=1,
          kernels=["convt_w", "first<u8>", "ps<1,2>", "ps<2,2>"]),
    _case("position-split-pn1-64x64", (32, 64), 64, 64, 1, {"wino_w": 0, "wino_ps": 4}, form="wino", nread=1,
          kernels=["convt_w", "first<u8>", "ps<1,1>", "ps<2,1>"]),
    _case("position-split-96x160-1", (32, 64), 96, 160, 1, {"wino_w": 0}, form="wino", nread=1,
          kernels=["convt_w", "first<u8>", "p<2,0,8,1>", "ps<1,1>", "ps<2,1>"]),
    _case("position-split-96x160-2", (32, 64), 96, 160, 2, {"wino_w": 0}, form="wino", nread=2,
          kernels=["convt_w", "first<u8>", "p<2,0,8,1>", "ps<1,2>", "ps<2,1>"]),
    _case("split-tiles-96x160", (32, 64), 96, 160, 4, {"precision": 1}, form="split", nread=4,
          kernels=["first<u8,split>", "h<1,0,16,2>", "h<2,0,16,2,SQ>", "h<2,0,8,3>", "h<2,1,8,3>", "head<split>"]),
    _case("split-padded-33x66-32x64", (33, 66), 32, 64, 4, {"precision": 1}, form="split", nread=4,
          kernels=["first<u8,split>", "h<1,0,16,2>", "h<1,0,8,3>", "h<2,0,16,2,SQ>", "h<2,1,8,3>", "head<split>"]),
    _case("split-tile-h8-96x160", (32, 64), 96, 160, 4, {"precision": 1, "tile_h": 8}, form="split", nread=4,
          kernels=["first<u8,split>", "h<1,0,8,3>", "h<2,0,8,3>", "h<2,1,8,3>", "head<split>"]),
    _case("split-h-square0-96x160", (32, 64), 96, 160, 4, {"precision": 1, "h_square": 0}, form="split", nread=4,
          kernels=["first<u8,split>", "h<1,0,16,2>", "h<2,0,16,2>", "h<2,0,8,3>", "h<2,1,8,3>", "head<split>"]),
    _case("split-bottleneck-1x1-16x16", (4, 8, 16, 32), 16, 16, 4, {"precision": 1}, form="split", nread=4,
          kernels=["first<u8,split>", "h<1,0,16,2>", "h<1,0,8,3>", "h<2,0,8,3>", "h<2,1,8,3>", "head<split>"]),
    _case("split-five-levels-64x96", (3, 6, 12, 24, 48), 64, 96, 4, {"precision": 1}, form="split", nread=4,
          kernels=["first<u8,split>", "h<1,0,16,2>", "h<1,0,8,3>", "h<2,0,8,3>", "h<2,1,8,3>", "head<split>"]),
    _case("split-fused-first-and-head-96x160", (32, 64), 96, 160, 16, {"precision": 1, "keep_taps": 0}, form="split", nread=4, fused_first=True, fused_head=True,
          kernels=["h<1,0,16,2>", "h<1,0,8,3,FIRST>", "h<1,0,8,3>", "h<2,0,16,2,SQ>", "h<2,0,8,3>", "h<2,1,8,3>"]),
    _case("direct-impl0-96x160", (32, 64), 96, 160, 4, {"wino": 0, "conv_impl": 0}, form="direct", nread=4,
          kernels=["first<u8>", "head", "mfma<1,0,8>", "mfma<2,0,8>", "mfma<2,1,8>"]),
    _case("fused-first-and-head-96x160", (32, 64), 96, 160, 16, {"wino": 0, "keep_taps": 0}, form="direct", nread=4, fused_first=True, fused_head=True,
          kernels=["o<1,0,8,3,FIRST>", "o<1,0,8,3>", "o<2,0,8,3>", "o<2,1,8,3>"]),
    _case("split-splitk-96x160-1", (32, 64), 96, 160, 1, {"precision": 1, "splitk": 1}, form="split", nread=1,
          kernels=["first<u8,split>", "h<1,0,16,2>", "h<1,0,8,3>+splitK", "h<2,0,16,2,SQ>", "h<2,0,8,3>+splitK", "h<2,1,8,3>+splitK", "head<split>"]),
    _case("splitk-nt1-0-33x66-1", (33, 66), 32, 64, 1, {"wino": 0, "splitk": 1, "splitk_nt1": 0}, form="direct", nread=1,
          kernels=["first<u8>", "head", "o<1,0,8,3>+splitK+reduce", "o<2,0,8,3>+splitK+reduce", "o<2,1,8,3>+splitK+reduce"]),
    _case("wave-split-wb2-64x64-1", (32, 64), 64, 64, 1, {"wino_w": 3}, form="wino", nread=1,
          kernels=["convt_w", "first<u8>", "w<2> nt=1", "w<2> nt=2"]),
    _case("wave-split-wp-33x66-1", (33, 66), 32, 64, 1, {}, form="wino", nread=1,
          kernels=["convt_w", "first<u8>", "head", "p<1,0,8,3>", "wp nt=2"]),
    _case("splitk-epilogue-33x66-8", (33, 66), 32, 64, 8, {"wino": 0, "splitk": 1, "splitk_fused": 0}, form="direct", nread=4,
          kernels=["epilogue<1,0,8>", "epilogue<2,0,8>", "epilogue<2,1,8>", "first<u8>", "head", "o<1,0,8,3>+splitK", "o<2,0,8,3>+splitK", "o<2,1,8,3>+splitK"]),
    # split K on the persistent kernel (conv_impl 1, or splitk_occ 0): raw accumulators of every K part, summed by k_splitk_epilogue
    _case("persistent-splitk-96x160-1", (32, 64), 96, 160, 1, {"wino": 0, "conv_impl": 1, "splitk": 1}, form="direct", nread=1,
          kernels=["epilogue<1,0,8>", "epilogue<2,0,8>", "epilogue<2,1,8>", "first<u8>", "p<1,0,8,3>", "p<1,0,8,3>+splitK", "p<2,0,8,1>",
                   "p<2,0,8,1>+splitK", "p<2,1,8,1>+splitK"]),
    _case("persistent-splitk-tps1-33x66-2", (33, 66), 32, 64, 2, {"wino": 0, "conv_impl": 1, "splitk": 1, "tps_nt1": 1}, form="direct", nread=2,
          kernels=["epilogue<1,0,8>", "epilogue<2,0,8>", "epilogue<2,1,8>", "first<u8>", "head", "p<1,0,8,1>+splitK", "p<2,0,8,1>+splitK",
                   "p<2,1,8,1>+splitK"]),
    _case("persistent-splitk-tps9-33x66-2", (33, 66), 32, 64, 2, {"wino": 0, "conv_impl": 1, "splitk": 1, "tps_nt1": 9, "tps_nt2": 3}, form="direct",
          nread=2, kernels=["epilogue<1,0,8>", "epilogue<2,0,8>", "epilogue<2,1,8>", "first<u8>", "head", "p<1,0,8,9>+splitK", "p<2,0,8,3>+splitK",
                            "p<2,1,8,1>+splitK"]),
]

# every kernel the f16 mode can launch, by the short label of its instantiation -> its text in og_unet_plan / in UNet.profile
F16_KERNELS = {
    "<2,0,16,2>": ("k_conv_mfma_f<2, 0, 16, 2, false, false>", "k_conv_mfma_f<2,0,16>"),
    "<2,0,16,2,SQ>": ("k_conv_mfma_f<2, 0, 16, 2, false, true>", "k_conv_mfma_f<2,0,16>"),
    "<1,0,16,2>": ("k_conv_mfma_f<1, 0, 16, 2, false, false>", "k_conv_mfma_f<1,0,16>"),
    "<2,0,8,3>": ("k_conv_mfma_f<2, 0, 8, 3, false, false>", "k_conv_mfma_f<2,0,8>"),
    "<1,0,8,3>": ("k_conv_mfma_f<1, 0, 8, 3, false, false>", "k_conv_mfma_f<1,0,8>"),
    "<2,1,8,3>": ("k_conv_mfma_f<2, 1, 8, 3, false, false>", "k_conv_mfma_f<2,1,8>"),
    "<1,0,8,3,FIRST>": ("k_conv_mfma_f<1, 0, 8, 3, true>", "k_conv_mfma_f<1,0,8,FIRST>"),
    "k_conv_first_f": ("k_conv_first_f", "k_conv_first_f<u8>"),
    "k_head_f": ("k_head_f", "k_head_f"),
}


def _f16(cid, feats, H, W, B, options, kernels, nread=2, fused_first=False, fused_head=False):
    opts = {"precision": 2}
    opts.update(options)
    return _case(cid, feats, H, W, B, opts, [F16_KERNELS[k][0] for k in kernels], form="f16", nread=nread, fused_first=fused_first,
                 fused_head=fused_head, prof=[F16_KERNELS[k][1] for k in kernels])


_F16_BIG = ["<2,0,16,2,SQ>", "<1,0,16,2>", "<2,1,8,3>"]
GPU_CASES += [
    _f16("f16-default-64", FULL, 256, 256, 64, {}, _F16_BIG + ["<1,0,8,3>", "k_conv_first_f"]),
    _f16("f16-fused-first-and-head-64", FULL, 256, 256, 64, {"keep_taps": 0}, _F16_BIG + ["<1,0,8,3>", "<1,0,8,3,FIRST>"],
         fused_first=True, fused_head=True),
    _f16("f16-default-1", FULL, 256, 256, 1, {}, _F16_BIG + ["<1,0,8,3>", "k_conv_first_f"], nread=1),
    _f16("f16-tile-h8-2", FULL, 256, 256, 2, {"tile_h": 8}, ["<2,0,8,3>", "<1,0,8,3>", "<2,1,8,3>", "k_conv_first_f"]),
    _f16("f16-h-square0-2", FULL, 256, 256, 2, {"h_square": 0}, ["<2,0,16,2>", "<1,0,16,2>", "<2,1,8,3>", "k_conv_first_f"]),
    _f16("f16-unfused-head-2", FULL, 256, 256, 2, {"fuse_head": 0}, _F16_BIG + ["k_conv_first_f", "k_head_f"]),
    _f16("f16-tiles-128x256", (32, 64), 128, 256, 64, {}, _F16_BIG + ["<1,0,8,3>", "k_conv_first_f"]),
    _f16("f16-tiles-96x160", (32, 64), 96, 160, 16, {}, _F16_BIG + ["<2,0,8,3>", "<1,0,8,3>", "k_conv_first_f"], nread=4),
    _f16("f16-padded-40x80-64x64", (40, 80), 64, 64, 8, {}, _F16_BIG + ["k_conv_first_f", "k_head_f"], nread=6),
    _f16("f16-padded-33x66-32x64", (33, 66), 32, 64, 4, {}, _F16_BIG + ["<1,0,8,3>", "k_conv_first_f", "k_head_f"], nread=4),
    _f16("f16-wide-96x192-64x128", (96, 192), 64, 128, 4, {}, _F16_BIG + ["k_conv_first_f", "k_head_f"], nread=4),
    _f16("f16-bottleneck-1x1-16x16", (4, 8, 16, 32), 16, 16, 4, {}, ["<2,0,8,3>", "<1,0,16,2>", "<1,0,8,3>", "<2,1,8,3>", "k_conv_first_f"], nread=4),
    _f16("f16-maps-1x16-16x256", (4, 8, 16, 32), 16, 256, 2, {}, ["<2,0,8,3>", "<1,0,16,2>", "<1,0,8,3>", "<2,1,8,3>", "k_conv_first_f"], nread=2),
    _f16("f16-five-levels-64x96", (3, 6, 12, 24, 48), 64, 96, 4, {}, ["<2,0,8,3>", "<1,0,16,2>", "<1,0,8,3>", "<2,1,8,3>", "k_conv_first_f"], nread=4),
    _f16("f16-large-512x512", (32, 64), 512, 512, 8, {}, _F16_BIG + ["<1,0,8,3>", "k_conv_first_f"], nread=1),
]


# new rows that are the only cover of no instantiation, overall or among the edge rows (tests/test_layer_ref.py checks that this list
# is exact: every other row added with the registry is the only cover of something) -> what the row adds instead
REDUNDANT_FOR_COVERAGE = {
    "persistent-tps9-33x66": "p<1,0,8,9> / p<2,0,8,3> on padded channels (33 -> 64, 66 -> 96) and every layer, not only 8-row tails",
    "position-split-pn1-64x64": "ps<1,1> / ps<2,1> forced on every layer of the 64 x 64 net (auto picks them on deep layers only)",
    "position-split-96x160-1": "the auto position split beside direct launches on maps that do not tile (24 x 40)",
    "position-split-96x160-2": "the same at two frames: ps<1,2>",
    "split-tiles-96x160": "the split-precision default on partial tiles",
    "split-tile-h8-96x160": "h<1,0,8,3> / h<2,0,8,3> on every layer of a net with partial tiles",
    "wave-split-wp-33x66-1": "wp nt=2 on padded channels, one frame per chain",
    "split-padded-33x66-32x64": "split precision with padded K",
    "split-bottleneck-1x1-16x16": "split precision down to a 1 x 1 bottleneck",
    "split-five-levels-64x96": "split precision on five levels and 3-channel layers",
}

# The NCHW-float entry point (``m(x)``: k_conv_first<float> / <float, true>) at precision 0 and 1: the six special frames at
# 64 x 64 (tests/test_gpu_layer_parity.py::test_f32_entry_point_in_f32_and_split_precision); ``entry_f32`` makes og_unet_plan and
# UNet.profile walk that entry point's chain
F32_ENTRY_CASES = [
    _case("entry-f32-33x66", (33, 66), 64, 64, 6, {"precision": 0, "entry_f32": 1}, form="wino", nread=6,
          kernels=["convt_w", "first<f32>", "head", "p<1,0,8,3>", "p<2,1,8,1>", "w<1> nt=1", "w<1> nt=2"]),
    _case("entry-f32-full", FULL, 64, 64, 6, {"precision": 0, "entry_f32": 1}, form="wino", nread=6,
          kernels=["convt_w", "first<f32>", "p<2,0,8,1>", "w<1> nt=1", "w<1> nt=2", "wp nt=2"]),
    _case("entry-f32-split-33x66", (33, 66), 64, 64, 6, {"precision": 1, "entry_f32": 1}, form="split", nread=6,
          kernels=["first<f32,split>", "h<1,0,16,2>", "h<2,0,16,2,SQ>", "h<2,1,8,3>", "head<split>"]),
    _case("entry-f32-split-full", FULL, 64, 64, 6, {"precision": 1, "entry_f32": 1}, form="split", nread=6,
          kernels=["first<f32,split>", "h<1,0,16,2>", "h<2,0,16,2,SQ>", "h<2,0,8,3>", "h<2,1,8,3>", "head<split>"]),
]


def kappa_of(form: str) -> dict:
    """kappa per op kind for a chain of the given form (the first layer, the transposed convs and the heads are direct in every
    f32 chain; split precision runs every op through the hi / lo arithmetic, the f16 mode through its own kernels)."""
    k, d = KAPPA[form], KAPPA["direct"]
    if form in ("split", "f16"):
        return {"first": k, "conv3": k, "convt": k, "head": k}
    return {"first": d, "conv3": k, "convt": d, "head": d}


def option_string(options: dict) -> str:
    return ",".join(f"{k}={v}" for k, v in options.items())


def plan_families(recs, B: int) -> set:
    """Kernel families of an og_unet_plan record list (``[{kernel, grid, ws, cnt, ...}]``) of a B-frame chain.  Pseudo-families:
    ``first-fused`` (downs.0 with the first layer inside), ``splitk-parts`` (a conv launch with more grid.z slices than frames:
    its K split over workgroups), ``splitk-fused-reduce`` (split parts with a workspace and arrival counters)."""
    import re

    out = set()
    for r in recs:
        k = r["kernel"]
        m = re.match(r"\(?\s*(k_\w+)", k)
        if m:
            out.add(m.group(1))
        if re.search(r"k_conv_mfma_[oh]<1, 0, 8, 3, true>", k):
            out.add("first-fused")
        if "k_conv_mfma" in k and r["grid"][2] > B:
            out.add("splitk-parts")
        if r["ws"] > 0 and r["cnt"] > 0 and "k_conv_mfma" in k:
            out.add("splitk-fused-reduce")
    return out


def plan_instantiations(recs) -> set:
    """Kernels of an og_unet_plan record list by instantiation, for all three arithmetic forms: every conv, transposed-conv,
    first-layer, head and split-K epilogue launch by the text the plan records for it, without parentheses.  What the record
    carries behind the instantiation is folded in where it names another code path, dropped where it does not: ``ksplit=N``
    becomes ``+splitK`` for N > 1 (as in ``UNet.profile``) and ``+splitK+reduce`` where the launch also has arrival counters (the
    last workgroup of a tile reduces the parts inside the kernel; without them ``k_splitk_epilogue`` follows), `` nt=N`` (the weight pack k_conv_wino_w / k_conv_wino_wp read: that
    of a 32- or of a 64-column layer) stays, the K walk of an f16 launch (`` chunks=N k_half=N``) goes.  The f16 mode's first-layer
    and head kernels stay without their arguments (``k_conv_first_f``, ``k_head_f``).  ``k_sum_counts`` (an exact integer sum
    behind the fused head, held by ``area == popcount(mask)``) is no layer kernel and is left out."""
    import re

    out = set()
    for r in recs:
        k = r["kernel"]
        m = re.match(r"\(?\s*(k_conv_first_f|k_head_f)\b", k)
        if m:
            out.add(m.group(1))
            continue
        m = re.match(r"\(?\s*(k_\w+(?:<[^>]*>)?)\)?(.*)$", k)
        if not m or m.group(1) == "k_sum_counts":
            continue
        inst, rest = m.group(1), m.group(2)
        nt = re.search(r" nt=(\d+)", rest)
        ks = re.search(r" ksplit=(\d+)", rest)
        split = "" if not ks or int(ks.group(1)) == 1 else "+splitK+reduce" if r["ws"] > 0 and r["cnt"] > 0 else "+splitK"
        out.add(inst + (f" nt={nt.group(1)}" if nt else "") + split)
    return out


def plan_half_chunks(recs) -> set:
    """Which kinds of half last chunk (``ConvArgs::k_half``) the f16 launches of a plan walk: ``"only"`` (the half chunk is the
    whole K loop) and / or ``"after-full"`` (it follows full 64-channel chunks)."""
    import re

    out = set()
    for r in recs:
        m = re.search(r"k_conv_mfma_f<.* chunks=(\d+) k_half=(\d+)", r["kernel"])
        if m and int(m.group(2)):
            out.add("only" if int(m.group(1)) == 1 else "after-full")
    return out


def profile_families(prof) -> set:
    """Kernel families of a ``UNet.profile`` list (its kernel names are the launch sites' labels)."""
    import re

    out = set()
    for p in prof:
        k = p["kernel"]
        m = re.match(r"(k_\w+)", k)
        if m:
            out.add(m.group(1))
        if "FIRST" in k:
            out.add("first-fused")
        if "+splitK" in k:
            out.add("splitK")
    return out


def profile_instantiations(prof) -> set:
    """The launch-site labels of a ``UNet.profile`` list, whole (``k_conv_mfma_f<2,0,16>``, ``k_conv_first_f<u8>``, ``k_head_f``)."""
    return {p["kernel"] for p in prof}
