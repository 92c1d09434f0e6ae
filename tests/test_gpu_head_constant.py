"""GPU (-m gpu): the U-Net head -- threshold, mask, gated count -- on CONSTANT logits, through every head form the options reach.

Head weight 0 makes every logit the head bias, in every form, so the decision point itself can be visited: logits of 0, +1e-9 (on
by sign, OFF by the f32 rule: tests/head_cases.py), -+1e-6, +-30; thresholds that ARE the probability; and all-on masks whose gated
area must be ``|box ∩ frame|`` exactly for boxes on every edge, corner and counting-block boundary.  The deciding launch of each
option set is named from ``og_unet_plan`` (``head_cases.HEAD_FORMS``: the last conv with the head fused into it -- Winograd,
wave-split Winograd, position-split, persistent, direct, split precision, f16 -- or ``k_head<false>`` / ``k_head<true>`` /
``k_head_f``); ``k_mask_area`` and ``k_resize_out`` count the same boxes.
"""
import numpy as np
import pytest

import head_cases as HC
import openglottal_amd as og
from openglottal_amd import geometry, synth

pytestmark = pytest.mark.gpu

FEATS = (4, 8, 16, 32)
SHAPES = [(96, 160), (64, 64)]     # 15 blocks of 1024 px whose boundaries fall inside rows; 4 blocks = one block of 4096 exactly
OPTIONS = list(HC.HEAD_FORMS)
_models = {}


def model(bias):
    if bias not in _models:
        sd = synth.make_unet_state_dict(FEATS, seed=5)
        sd["head.weight"] = np.zeros_like(sd["head.weight"])
        sd["head.bias"] = np.full_like(sd["head.bias"], bias)
        m = og.UNet(1, 1, FEATS)
        m.load_state_dict(sd)
        m.to("cuda:0").eval()
        m.set_chunk(128)                                             # every call below is one micro-batch: the plan's B is the call's
        assert m.chunk == 128
        _models[bias] = m
    return _models[bias]


def frames(B, H, W):
    return synth.random_gray_frames(B, H, W, seed=H + W)


def kernel_of(options, B, H, W):
    import torch

    assert torch.cuda.get_device_properties(0).multi_processor_count == 256    # og_unet_plan walks the decisions of a 256-CU chip
    k = HC.head_kernel(FEATS, B, H, W, options)
    small, full = HC.HEAD_FORMS[options]
    assert k.startswith(small if B == 1 else full), (options, B, k)
    return k


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ───────────────────────────── the table: logits == bias, mask by the f32 rule ─────────────────────────────

TABLE = [(0.0, False), (1e-9, False), (-1e-6, False), (1e-6, True), (30.0, True), (-30.0, False)]


@pytest.mark.parametrize("options", OPTIONS, ids=[o or "defaults" for o in OPTIONS])
@pytest.mark.parametrize("bias,on", TABLE, ids=[f"{b:+g}" for b, _ in TABLE])
def test_constant_logits_equal_the_bias_and_the_mask_follows_the_f32_rule(bias, on, options):
    m = model(bias)
    HC.set_options(m, options)
    try:
        for H, W in SHAPES:
            for B in (1, 40):
                k = kernel_of(options, B, H, W)
                mask, area, logits = m.segment(frames(B, H, W), want_logits=True)
                assert np.all(bits(logits) == bits(np.float32(bias))), (options, k, np.unique(logits)[:4])
                assert HC.check_mask_follows_the_rule(mask > 0, logits, (options, k)) == 0     # (no table entry is in the undecided window)
                assert np.all(mask == (255 if on else 0)), (options, k, bias, np.unique(mask))
                assert area.tolist() == [H * W if on else 0] * B, (options, k, bias)
                print(f"bias {bias:+g} [{options or 'defaults'}] {H}x{W} B={B}: {k}: logits == bias bit for bit, mask all {'on' if on else 'off'}")
    finally:
        HC.set_options(m, "")


# ───────────────────────────── thresholds that are the probability ─────────────────────────────


def constant_prob(m, H, W):
    """f32 sigmoid of the constant logit as the device computes it: ``segment_resized(..., want_prob=True)`` at network size."""
    _, _, prob = m.segment_resized(frames(1, H, W), net=(H, W), want_prob=True)
    assert len(np.unique(bits(prob))) == 1
    return np.float32(prob.flat[0])


@pytest.mark.parametrize("options", OPTIONS, ids=[o or "defaults" for o in OPTIONS])
@pytest.mark.parametrize("bias", [0.0, 0.3, -0.7, 1e-6, 5.0], ids=lambda b: f"{b:+g}")
def test_the_threshold_is_strict_at_the_probability_itself(bias, options):
    m = model(bias)
    H, W = SHAPES[0]
    p = constant_prob(m, H, W)
    p64 = 1.0 / (1.0 + np.exp(-np.float64(np.float32(bias))))
    assert abs(float(p) - p64) <= 4 * float(np.spacing(np.float32(p64))), (p, p64)     # (tests/test_gpu_resized.py's bound on expf)
    below = np.nextafter(p, np.float32(0))
    HC.set_options(m, options)
    try:
        for B in (1, 40):
            k = kernel_of(options, B, H, W)
            fr = frames(B, H, W)
            mask, area, _ = m.segment(fr, threshold=float(p))
            assert not mask.any() and not area.any(), (options, k, bias, "threshold = p must switch every pixel off")
            mask, area, _ = m.segment(fr, threshold=float(below))
            assert mask.all() and area.tolist() == [H * W] * B, (options, k, bias, "threshold = nextafter(p, 0) must switch every pixel on")
        print(f"bias {bias:+g} [{options or 'defaults'}] {k}: p = {p!r}: all off at p, all on at nextafter(p, 0)")
    finally:
        HC.set_options(m, "")


# ───────────────────────────── all-on masks: area == |box ∩ frame| ─────────────────────────────


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("options", OPTIONS, ids=[o or "defaults" for o in OPTIONS])
def test_gated_area_of_an_all_on_mask_is_the_box_cut_to_the_frame(options, shape):
    H, W = shape
    m = model(30.0)
    boxes = HC.box_list(H, W)
    want = [HC.box_area(b, H, W) for b in boxes]
    assert 0 in want and H * W in want and 1 in want and W in want
    n = len(boxes)
    fr = frames(n, H, W)
    HC.set_options(m, options)
    try:
        k = kernel_of(options, n, H, W)
        mask, area, _ = m.segment(fr, boxes=boxes)
        assert mask.all()
        assert area.tolist() == want, (options, k, [(b.tolist(), int(a), w) for b, a, w in zip(boxes, area, want) if a != w][:5])
        _, area, _ = m.segment(fr, boxes=boxes, want_mask=False)     # the count alone
        assert area.tolist() == want, (options, k)
        _, area, _ = m.segment(fr)                                   # no boxes at all: the whole frame
        assert area.tolist() == [H * W] * n
        k1 = kernel_of(options, 1, H, W)
        for i in range(n):                                           # one frame per call: the small-launch form, mask and area
            _, a1, _ = m.segment(fr[i:i + 1], boxes=boxes[i:i + 1])  # written to pinned memory by the kernel
            assert int(a1[0]) == want[i], (options, k1, boxes[i].tolist(), int(a1[0]), want[i])
        print(f"all-on {H}x{W} [{options or 'defaults'}]: {n} boxes, area == |box ∩ frame| through {k} (one call) and {k1} (one frame per call)")
    finally:
        HC.set_options(m, "")


@pytest.mark.parametrize("shape", SHAPES + [(100, 120)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_k_mask_area_counts_the_same_boxes_on_a_resident_mask(shape):
    import torch

    H, W = shape
    m = model(30.0)
    boxes = HC.box_list(H, W)
    n = len(boxes)
    want = [HC.box_area(b, H, W) for b in boxes]
    if H % 16 == 0 and W % 16 == 0:      # the mask the head left on the device
        d_mask = torch.empty((n, H, W), dtype=torch.uint8, device="cuda:0")
        d_area = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        m.segment_dev(torch.from_numpy(frames(n, H, W)).to("cuda:0"), n, H, W, d_area, 0.5, None, d_mask)
        m.sync()
        assert bool((d_mask == 255).all())
    else:                                # a frame size only the resized path takes: 12 000 px, the last block of 4096 partial
        d_mask = torch.full((n, H, W), 255, dtype=torch.uint8, device="cuda:0")
    out = torch.full((n,), -7, dtype=torch.int32, device="cuda:0")
    m.mask_area_dev(d_mask, n, H, W, torch.from_numpy(boxes).to("cuda:0"), out)
    m.sync()
    assert out.cpu().tolist() == want, [(b.tolist(), int(a), w) for b, a, w in zip(boxes, out.cpu(), want) if a != w][:5]
    m.mask_area_dev(d_mask, n, H, W, None, out)
    m.sync()
    assert out.cpu().tolist() == [H * W] * n
    print(f"k_mask_area {H}x{W}: {n} boxes, area == |box ∩ frame|")


# ───────────────────────────── frames of another size: k_resize_out ─────────────────────────────


@pytest.mark.parametrize("options", ["", "fuse_head=0", "precision=2"], ids=["defaults", "fuse_head=0", "precision=2"])
@pytest.mark.parametrize("shape", [(100, 120), (96, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_resized_frames_threshold_the_host_resize_of_the_constant_probability(shape, options):
    """``segment_resized`` (u8 -> 256x256 -> U-Net -> sigmoid -> back to HxW in f32 -> strict >): the expected mask is
    ``geometry.resize_linear`` of the constant network-size probability, which may round off ``p`` (``p (1 - f) + p f``)."""
    H, W = shape
    fr = frames(2, H, W)
    for bias in (0.3, -0.7):
        m = model(bias)
        p = constant_prob(m, 256, 256)
        want_prob = geometry.resize_linear(np.full((256, 256), p, np.float32), W, H)
        lo, hi = np.float32(want_prob.min()), np.float32(want_prob.max())
        HC.set_options(m, options)
        try:
            for thr in (0.5, p, np.nextafter(p, np.float32(0)), hi, np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(0))):
                mask, area, prob = m.segment_resized(fr, net=256, threshold=float(thr), want_prob=True)
                assert np.array_equal(bits(prob), bits(np.stack([want_prob] * 2))), (shape, options, bias)
                on = want_prob > np.float32(thr)
                assert np.array_equal(mask > 0, np.stack([on] * 2)), (shape, options, bias, thr)
                assert area.tolist() == [int(on.sum())] * 2
                mask2, area2 = m.segment_resized(fr, net=256, threshold=float(thr))          # the streamed entry
                assert np.array_equal(mask2, mask) and np.array_equal(area2, area)
        finally:
            HC.set_options(m, "")
        print(f"resized {H}x{W} [{options or 'defaults'}] bias {bias:+g}: p {p!r}, host resize in [{lo!r}, {hi!r}] "
              f"({len(np.unique(want_prob))} distinct values): masks follow it at six thresholds")
    # all on: the count inside source-coordinate boxes, on every edge and block boundary of the source frame
    m = model(30.0)
    boxes = HC.box_list(H, W)
    want = [HC.box_area(b, H, W) for b in boxes]
    HC.set_options(m, options)
    try:
        mask, area = m.segment_resized(frames(len(boxes), H, W), net=256, boxes=boxes)
        assert mask.all() and area.tolist() == want, [(b.tolist(), int(a), w) for b, a, w in zip(boxes, area, want) if a != w][:5]
    finally:
        HC.set_options(m, "")
    print(f"resized {H}x{W} [{options or 'defaults'}] all on: {len(boxes)} boxes, area == |box ∩ frame| through k_resize_out")
