"""The U-Net head's decision rule and gated count, stated once for tests/test_gpu_head_constant.py and tests/test_gpu_f16.py.

THE RULE (every head form, ``k_resize_out``, and the reference's f32 ``torch.sigmoid(x) > thr``): a pixel is on iff
``prob > thr`` with ``prob = 1.0f / (1.0f + expf(-logit))`` in f32 -- strict, and decided on the ROUNDED probability, not on the sign
of the logit.  At ``thr = 0.5`` by bit reasoning:

* ``logit < 2^-25`` (zero, negative, and positive below 2^-25): the true ``exp(-logit)`` is above ``1 - 2^-25``, an expf within one
  ulp (2^-24 below 1) returns ``1 - 2^-24`` or more, so ``1 + e`` rounds to 2 or more (``2 - 2^-24`` is a tie and goes to the even
  2.0), ``prob <= 0.5``: OFF.  A positive logit there is off although its sign says on.
* ``logit >= 2^-21``: an expf within 4 ulp gives ``e <= 1 - 2^-21 + 4 * 2^-24 = 1 - 2^-22``, ``1 + e <= 2 - 2^-22`` exactly,
  ``prob >= 0.5 + 2^-24``: ON.
* in between (six ten-millionths wide) the outcome depends on the last bits of expf and is left to the device's own ``prob``.
"""
import ctypes as C

import numpy as np

from openglottal_amd._lib import lib

OFF_BELOW = 2.0 ** -25
ON_FROM = 2.0 ** -21


def check_mask_follows_the_rule(on, logits, what=""):
    """``on`` (bool) against f32 ``logits`` at threshold 0.5; returns the number of pixels in the undecided window."""
    on, lg = np.asarray(on, bool), np.asarray(logits, np.float32)
    assert not np.isnan(lg).any(), what
    assert not on[lg < OFF_BELOW].any(), (what, "on although prob_f32 <= 0.5", int(on[lg < OFF_BELOW].sum()))
    assert on[lg >= ON_FROM].all(), (what, "off although prob_f32 > 0.5", int((~on[lg >= ON_FROM]).sum()))
    return int(((lg >= OFF_BELOW) & (lg < ON_FROM)).sum())


def box_area(box, H, W) -> int:
    """``|box ∩ frame|`` as every counting kernel gates it: x1 < 0 is `no detection`, an empty or inverted box counts nothing."""
    if box is None:
        return H * W
    x1, y1, x2, y2 = (int(v) for v in box)
    if x1 < 0:
        return 0
    return max(0, min(x2, W) - max(x1, 0)) * max(0, min(y2, H) - max(y1, 0))


def box_list(H, W) -> np.ndarray:
    """int32 ``[n,4]``: no detection, the full frame, every edge and corner, one pixel, empty, inverted, past the right and bottom
    edges, and for every multiple of 1024 pixels (the block of ``k_head``; every fourth is a block of ``k_mask_area``) the row that
    holds it, and that row cut at it."""
    b = [(-1, -1, -1, -1), (-1, 0, W, H), (0, 0, W, H),
         (0, 0, W, 1), (0, H - 1, W, H), (0, 0, 1, H), (W - 1, 0, W, H),                                  # edges
         (0, 0, 3, 2), (W - 3, 0, W, 2), (0, H - 2, 3, H), (W - 3, H - 2, W, H),                          # corners
         (W // 2, H // 2, W // 2 + 1, H // 2 + 1), (0, 0, 1, 1), (W - 1, H - 1, W, H),                    # one pixel
         (5, 7, 5, 20), (5, 7, 30, 7), (30, 7, 5, 20), (5, 20, 30, 7), (W, 0, W + 9, H), (0, H, W, H + 9),  # empty, inverted, outside
         (W // 3, H // 4, W + 40, H // 2), (W // 3, H // 4, W // 2, H + 40), (1, 1, W + 1, H + 1), (0, 0, 1 << 20, 1 << 20)]
    for p in range(1024, H * W, 1024):
        y, x = divmod(p, W)
        b.append((0, y, W, y + 1))
        if x:
            b += [(0, y, x, y + 1), (x, y, W, y + 1)]
        else:
            b.append((0, y - 1, W, y + 1))
    return np.array(b, np.int32)


def head_kernel(feats, B, H, W, options="") -> str:
    """The launch that decides the mask in ``og_unet_plan``'s chain for these options: ``k_head<false>`` / ``k_head<true>`` /
    ``k_head_f``, or the last conv (the head fused into its epilogue) in front of ``k_sum_counts``."""
    f = (C.c_int * len(feats))(*feats)
    buf = C.create_string_buffer(1 << 16)
    n = lib().og_unet_plan(f, len(feats), B, H, W, 1, options.encode(), buf, len(buf), None)
    assert n > 0, (n, options)
    k = [line.rsplit("|", 7)[0] for line in buf.value.decode().strip().split("\n")]
    if k[-1].startswith("k_head"):
        return k[-1]
    assert k[-1] == "k_sum_counts" and k[-2].startswith(("k_conv", "(k_conv")), k[-3:]
    return k[-2] + " +head"


# option sets -> the family of the deciding launch at one frame per call and at a chip-filling call (og_unet_plan at 256 CUs names the
# instantiation; the test asserts the family, so that the list of head forms is shown closed)
HEAD_FORMS = {
    "": ("k_conv_wino_w", "k_conv_wino<1>"),
    "wino_w=0": ("k_conv_wino_ps<1", "k_conv_wino<1>"),
    "wino_w=2": ("k_conv_wino_w<1>", "k_conv_wino_w<1>"),
    "wino_w=3": ("k_conv_wino_w<2>", "k_conv_wino_w<2>"),
    "wino_w=4": ("k_conv_wino_wp", ("k_conv_wino_wp", "k_conv_wino_w<1>")),   # (the position split while its workspace holds the tiles)
    "wino=0": ("k_conv_mfma_p<1, 0, 8, 3>", "k_conv_mfma_o<1, 0, 8, 3,"),
    "conv_impl=1": ("k_conv_mfma_p<1, 0, 8, 3>", "k_conv_mfma_p<1, 0, 8, 3>"),
    "conv_impl=3": ("k_conv_mfma_o<1, 0, 8, 4,", "k_conv_mfma_o<1, 0, 8, 4,"),
    "conv_impl=0": ("k_head<false>", "k_head<false>"),
    "fuse_head=0": ("k_head<false>", "k_head<false>"),
    "precision=1": ("k_conv_mfma_h<1, 0, 8, 3,", "k_conv_mfma_h<1, 0, 8, 3,"),
    "precision=1,fuse_head=0": ("k_head<true>", "k_head<true>"),
    "precision=2": ("(k_conv_mfma_f<1, 0, 8, 3,", "(k_conv_mfma_f<1, 0, 8, 3,"),
    "precision=2,fuse_head=0": ("k_head_f", "k_head_f"),
}
OPTION_DEFAULTS = dict(wino=1, wino_w=1, conv_impl=2, fuse_head=1, precision=0)


def set_options(m, options: str):
    """Back to the defaults, then ``options`` (precision last: it re-plans the arena)."""
    want = dict(OPTION_DEFAULTS)
    want.update({kv.split("=")[0]: int(kv.split("=")[1]) for kv in filter(None, options.split(","))})
    for k, v in want.items():
        m.set_option(k, v)
