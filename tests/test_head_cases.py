"""CPU: what tests/test_gpu_head_constant.py takes from tests/head_cases.py holds without a device -- the box list's expected areas
are numpy's slices of an all-on frame, the closed list of head forms is what ``og_unet_plan`` walks for every option set and call
size the GPU test uses, and the f32 decision rule's two windows are what numpy's own f32 sigmoid gives."""
import numpy as np
import pytest

import head_cases as HC

FEATS = (4, 8, 16, 32)
SHAPES = [(96, 160), (64, 64)]


@pytest.mark.parametrize("shape", SHAPES + [(100, 120)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_box_areas_are_numpy_slices_of_an_all_on_frame(shape):
    H, W = shape
    on = np.ones((H, W), bool)
    boxes = HC.box_list(H, W)
    assert boxes.dtype == np.int32 and len({tuple(b) for b in boxes.tolist()}) == len(boxes)
    for b in boxes:
        x1, y1, x2, y2 = b.tolist()
        want = 0 if x1 < 0 else int(on[y1:y2, x1:x2].sum())          # (no box of the list has a negative y1: slices do not wrap)
        assert y1 >= 0 or x1 < 0
        assert HC.box_area(b, H, W) == want, b
    assert HC.box_area(None, H, W) == H * W
    # every multiple of 1024 pixels (and so of 4096) has its row, and the row cut at it
    for p in range(1024, H * W, 1024):
        y, x = divmod(p, W)
        assert (0, y, W, y + 1) in [tuple(b) for b in boxes.tolist()]
        assert x == 0 or (0, y, x, y + 1) in [tuple(b) for b in boxes.tolist()]


@pytest.mark.parametrize("options", list(HC.HEAD_FORMS), ids=[o or "defaults" for o in HC.HEAD_FORMS])
def test_the_list_of_head_forms_is_the_plan(options):
    small, full = HC.HEAD_FORMS[options]
    for H, W in SHAPES:
        for B in (1, 40, len(HC.box_list(H, W))):
            k = HC.head_kernel(FEATS, B, H, W, options)
            print(f"[{options or 'defaults'}] {H}x{W} B={B}: {k}")
            assert k.startswith(small if B == 1 else full), (options, B, k)
    kinds = {k for pair in HC.HEAD_FORMS.values() for v in pair for k in ((v,) if isinstance(v, str) else v)}
    for form in ("k_conv_wino<1>", "k_conv_wino_w<1>", "k_conv_wino_w<2>", "k_conv_wino_wp", "k_conv_wino_ps<1", "k_conv_mfma_p<", "k_conv_mfma_o<",
                 "k_conv_mfma_h<", "(k_conv_mfma_f<", "k_head<false>", "k_head<true>", "k_head_f"):
        assert any(k.startswith(form) for k in kinds), form


def test_the_two_windows_of_the_f32_rule():
    def on(lg):
        lg = np.asarray(lg, np.float32)
        return (np.float32(1) / (np.float32(1) + np.exp(-lg))) > np.float32(0.5)

    below = np.array([0.0, -0.0, -1e-6, -30.0, 1e-9, 2.0 ** -26, np.nextafter(np.float32(HC.OFF_BELOW), np.float32(0)), 1e-38], np.float32)
    above = np.array([HC.ON_FROM, 1e-6, 1.0, 30.0, 88.0], np.float32)
    assert not on(below).any() and on(above).all()
    assert HC.check_mask_follows_the_rule(on(np.concatenate([below, above])), np.concatenate([below, above])) == 0
    with pytest.raises(AssertionError):                              # `logits > 0`, the statement this replaces, fails it
        HC.check_mask_follows_the_rule(below > 0, below)
    assert HC.check_mask_follows_the_rule(np.array([True, False]), np.array([1e-7, 1e-7], np.float32)) == 2
