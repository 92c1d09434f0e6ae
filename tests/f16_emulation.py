"""CPU emulation of the f16 inference mode (`set_option("precision", 2)`).  TEST INFRASTRUCTURE: the product never imports it.

It restates the mode's arithmetic with torch on the CPU and rounds exactly where the library rounds:

* weights of every 3x3 conv and transposed conv to f16 (round to nearest even, once); BN stays f32 (eval mode);
* every activation a later layer reads to f16, once, after BN + ReLU (after the bias for transposed convs); max-pool of the
  rounded values (= the rounded max);
* first layer (Cin = 1) in f32, output rounded; the last conv's output rounded BEFORE the head; head in f32, f32 logits;
* accumulation in f32 (products of two f16 values are exact in f32; only the order of the sums is torch's, not the GPU's).

`half=False` is the plain f32 forward (the repository's oracle, op for op), so the same code pins itself to the reference
fixtures.  `channels_last=True` runs the same network in torch's NHWC kernels: another summation order, which is what the
f16 rounding is sensitive to -- the difference between the two orders measures how far a THIRD order (the GPU's) may lie.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_oracle as O

BN_EPS = O.BN_EPS


def _q(x):
    return x.half().float()


def forward(sd_t, x, half=True, channels_last=False, taps=None):
    """sd_t: state_dict of torch f32 tensors; x [B,1,H,W] f32 -> logits [B,1,H,W] f32.  taps: dict filled with the oracle's
    layer names ("downs.0.a", "pool0", "ups.0", ..., "head") -> the values a later layer reads (rounded when half)."""
    r = _q if half else (lambda t: t)
    fmt = torch.channels_last if channels_last else torch.contiguous_format

    def tap(name, v):
        if taps is not None:
            taps[name] = v.contiguous().numpy().copy()

    def dc(x, p):
        for c, n, s in (("0", "1", ".a"), ("3", "4", ".b")):
            w = sd_t[f"{p}.net.{c}.weight"]
            first = w.shape[1] == 1 and p == "downs.0"   # the first layer stays an f32 fma chain
            x = F.conv2d(x.contiguous(memory_format=fmt), (w if first else r(w)).contiguous(memory_format=fmt), None, 1, 1)
            x = F.batch_norm(x, sd_t[f"{p}.net.{n}.running_mean"], sd_t[f"{p}.net.{n}.running_var"],
                             sd_t[f"{p}.net.{n}.weight"], sd_t[f"{p}.net.{n}.bias"], False, 0.1, BN_EPS)
            x = r(F.relu(x))
            tap(p + s, x)
        return x

    L = O.n_levels(sd_t)
    skips = []
    for i in range(L):
        x = dc(x, f"downs.{i}")
        skips.append(x)
        x = F.max_pool2d(x, 2, 2)
        tap(f"pool{i}", x)
    x = dc(x, "bottleneck")
    for j in range(L):
        x = r(F.conv_transpose2d(x.contiguous(memory_format=fmt), r(sd_t[f"ups.{2 * j}.weight"]), sd_t[f"ups.{2 * j}.bias"], 2))
        tap(f"ups.{2 * j}", x)
        x = torch.cat([skips[-(j + 1)], x], dim=1)
        x = dc(x, f"ups.{2 * j + 1}")
    out = F.conv2d(x.contiguous(memory_format=fmt), sd_t["head.weight"].contiguous(memory_format=fmt), sd_t["head.bias"])
    tap("head", out)
    return out.contiguous()


def logits(sd, frames_u8, half=True, channels_last=False, batch=16):
    """state_dict of numpy arrays, frames [B,H,W] u8 (at network size) -> logits [B,H,W] f32."""
    sd_t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in sd.items()}
    x = torch.from_numpy(frames_u8.astype("float32") / 255.0)[:, None]
    with torch.no_grad():
        return torch.cat([forward(sd_t, x[i:i + batch], half, channels_last) for i in range(0, len(x), batch)])[:, 0].numpy()


def layer_taps(sd, x_f32, half=True, channels_last=False):
    """x [B,1,H,W] f32 -> {layer name: [B,C,H,W] f32} (the names of tests/golden/unet_small_layers.npz), head included."""
    sd_t = {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in sd.items()}
    taps = {}
    with torch.no_grad():
        forward(sd_t, torch.from_numpy(np.ascontiguousarray(x_f32, dtype=np.float32)), half, channels_last, taps)
    return taps


def masks_from_logits(lg):
    """The reference's threshold: sigmoid(logit) > 0.5 in f32 (utils.py:237-241) -> bool."""
    with torch.no_grad():
        return (torch.sigmoid(torch.from_numpy(np.ascontiguousarray(lg))) > 0.5).numpy()


def emulation_error(sd, frames_u8, ref_logits):
    """(E, D, lg_nchw, lg_nhwc): E = max |emulation - reference| over both memory formats, D = max |NCHW - NHWC| of the emulation."""
    a = logits(sd, frames_u8, True, False)
    b = logits(sd, frames_u8, True, True)
    e = max(float(np.abs(a - ref_logits).max()), float(np.abs(b - ref_logits).max()))
    return e, float(np.abs(a - b).max()), a, b
