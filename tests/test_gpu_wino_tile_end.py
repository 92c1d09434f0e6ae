"""GPU (-m gpu): the tile end of k_conv_wino<1> / <2> (output transform on accumulator register pairs + wino_tile_end) against
its twins, which still finish a tile through conv_epilogue_b, and against the float64 layer reference.

Seeded net (32, 64, 128, 256) on frames of 64 x 64, 128 x 64 and 64 x 128 pixels, B = 1 and 3.  At these sizes the chain runs
k_conv_wino<1> with the pooled output (downs.0.b), without it (ups.7.a) and with the fused head (ups.7.b), and k_conv_wino<2> with
(downs.1.b, downs.2.b) and without the pooled output (downs.1.a, downs.2.a, ups.3.*, ups.5.*): <2> at one tile per frame (the
16 x 16 map of the 64 x 64 frames) and at 2 to 8 in x, in y or in both, <1> at 8 to 16 -- the non-square shapes tell a swapped row / column
offset from a right one.  Two handles: the DEFAULT one takes the twins at these batch sizes (k_conv_wino_w / _wp: launches that
cannot fill the chip), the FORCED one (options wino_w 0, wino_ps 0) runs k_conv_wino itself; which kernels ran is asserted
through UNet.profile.

  (a) every layer tensor of the forced handle is array_equal to the default handle's (keep_taps 1: the fused head also stores the
      last activation -- wino_tile_end's HEAD 2 copy);
  (b) every layer tensor is within oracle.layer_ref's bound for the "wino" form (kappa 24 on conv layers), applied as
      tests/test_gpu_layer_parity.py applies it: check_net on the forced handle's tensors; by (a) the default handle's are the same
      numbers;
  (c) area, mask and logits of segment_dev are array_equal between the handles with the fused head on (keep_taps 0: the HEAD 1
      copy, no activation stored) and off (k_head behind the HEAD 0 copy), with boxes_dev set and unset, and with the optional
      outputs left out (areas only: logits and mask go to a buffer of zero records).
"""
import numpy as np
import pytest

import openglottal_amd as og
from openglottal_amd import synth
from oracle import layer_ref as R

pytestmark = pytest.mark.gpu

FEATS = (32, 64, 128, 256)
SHAPES = [(64, 64), (128, 64), (64, 128)]


def frames_of(H, W, B):
    sp = R.special_frames(H, W, seed=7)
    return np.ascontiguousarray(np.concatenate([sp["mosaic"][None], synth.random_gray_frames(2, H, W, seed=8)])[:B])


def handle(sd, B, forced):
    m = og.UNet(1, 1, FEATS)
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    if forced:
        m.set_option("wino_w", 0)
        m.set_option("wino_ps", 0)
    m.set_chunk(B)
    return m


@pytest.fixture(scope="module")
def sd():
    return synth.make_unet_state_dict(FEATS, seed=11, head_scale=3.0, head_bias=-0.5)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_tile_end_matches_twins_and_float64(sd, H, W, B):
    import torch

    gray = frames_of(H, W, B)
    dev = torch.device("cuda", 0)
    gdev = torch.from_numpy(gray).to(dev)
    forced, default = handle(sd, B, True), handle(sd, B, False)

    # which kernels: the forced handle runs k_conv_wino on every layer the default handle gives to a twin
    kf = [p["kernel"] for p in forced.profile(gdev, B, H, W, reps=1)]
    kd = [p["kernel"] for p in default.profile(gdev, B, H, W, reps=1)]
    assert "k_conv_wino<1>" in kf and "k_conv_wino<2>" in kf and not any(k.startswith("k_conv_wino_") for k in kf), kf
    assert not any(k.startswith("k_conv_wino<") for k in kd) and any(k.startswith("k_conv_wino_w") for k in kd), kd
    assert len(kf) == len(kd) and all(a.startswith("k_conv_wino<") for a, b in zip(kf, kd) if b.startswith("k_conv_wino_")), (kf, kd)

    # (a) + (b): all taps, fused head with the activation stored
    out = {}
    for name, m in (("forced", forced), ("default", default)):
        m.set_option("keep_taps", 1)
        masks, areas, logits = m.segment(gray, want_logits=True)
        out[name] = (masks, areas, logits, {n: m.activation(n, B) for n in R.layer_names(len(FEATS))})
    for n in R.layer_names(len(FEATS)):
        assert np.array_equal(out["forced"][3][n], out["default"][3][n]), n
    for i in range(3):
        assert np.array_equal(out["forced"][i], out["default"][i]), ("masks", "areas", "logits")[i]
    masks, areas, logits, taps = out["forced"]
    worst = R.check_net(sd, gray, taps.__getitem__, logits, R.kappa_of("wino"), mask=masks, area=areas, form="wino")
    print(f"{H}x{W} B={B} [wino kappa {R.KAPPA['wino']:g}] worst |err|/bound per layer: "
          + " ".join(f"{k}={v:.3f}" for k, v in worst.items() if not k.startswith("pool")) + f"  (max {max(worst.values()):.3f})")

    # (c): the device entry point, fused head on / off, boxes set / unset, optional outputs present / left out
    boxes = np.array([[5, 9, W - 7, H - 3], [-1, -1, -1, -1], [W // 2, 0, W, H // 2 + 1]], np.int32)[:B]
    bdev = torch.from_numpy(np.ascontiguousarray(boxes)).to(dev)
    for fuse in (1, 0):
        for bx in (None, bdev):
            got = {}
            for name, m in (("forced", forced), ("default", default)):
                m.set_option("keep_taps", 0)
                m.set_option("fuse_head", fuse)
                area = torch.full((B,), -1, dtype=torch.int32, device=dev)
                mask = torch.full((B, H, W), 7, dtype=torch.uint8, device=dev)
                lg = torch.full((B, H, W), -7.0, dtype=torch.float32, device=dev)
                m.segment_dev(gdev, B, H, W, area, boxes_dev=bx, mask_dev=mask, logits_dev=lg)
                area_only = torch.full((B,), -1, dtype=torch.int32, device=dev)
                m.segment_dev(gdev, B, H, W, area_only, boxes_dev=bx)
                m.sync()
                got[name] = (area.cpu().numpy(), mask.cpu().numpy(), lg.cpu().numpy(), area_only.cpu().numpy())
            for i, what in enumerate(("area", "mask", "logits", "area (no mask, no logits)")):
                assert np.array_equal(got["forced"][i], got["default"][i]), (what, fuse, bx is not None)
            a, mk, lgt, a2 = got["forced"]
            assert np.array_equal(a, a2) and np.array_equal(lgt, logits) and np.array_equal(mk, masks), (fuse, bx is not None)
            exp = []
            for b in range(B):
                x1, y1, x2, y2 = (0, 0, W, H) if bx is None else boxes[b]
                exp.append(0 if x1 < 0 else int((mk[b, y1:y2, x1:x2] > 0).sum()))
            assert np.array_equal(a, np.array(exp, np.int32)), (a, exp, fuse, bx is not None)
