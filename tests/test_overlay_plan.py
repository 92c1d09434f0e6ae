"""og_overlay_plan: the launches, grids and workspace of the streamed overlay pass, walked without a GPU.  Style none is k_overlay
alone; the outlined styles label the outside background first (the tiled blob filter's four launches on whole-frame windows), then
k_overlay; the workspace is that of one micro-batch, and the writes column ends at B * H * W * 3."""
import ctypes as C

import pytest

from openglottal_amd import overlay as OV
from openglottal_amd._lib import OpenGlottalHipError, lib

MiB = 1 << 20
T = int(lib().og_classic_tiled_limit(1))
LABEL_CHAIN = ("k_tblob_background_mask", "k_tblob_seams<false>", "k_tblob_flatten", "k_tblob_border")


def micro_batch(chunk, H, W):
    return max(1, min(chunk, (64 * MiB) // (H * W * 3)))


CASES = [(1, 33, 33, 1, 32), (5, 2 * T + 3, T + 5, 3, 2), (70, 256, 256, 3, 32), (9, 480, 640, 1, 128), (300, 480, 640, 3, 128),
         (3, 1080, 1920, 3, 128), (7, 300, 260, 1, 1024)]


@pytest.mark.parametrize("B,H,W,ch,chunk", CASES)
@pytest.mark.parametrize("style", ("none", "contour", "fill"))
def test_plan_lists_each_kernel_with_its_grid(style, B, H, W, ch, chunk):
    recs, ws = OV.plan(B, H, W, ch, chunk, style)
    mb = micro_batch(chunk, H, W)
    n_batches = -(-B // mb)
    chain_names = (() if style == "none" else LABEL_CHAIN) + (f"k_overlay<{ch}>",)
    L = len(chain_names)
    assert L == (1 if style == "none" else 5) and len(recs) == L * n_batches
    tiles = -(-H // T) * -(-W // T)
    px = -(-(H * W) // 256)
    gz_limit = lib().og_workspace_limit(2)
    left, done = B, 0
    for k in range(n_batches):
        nb = min(mb, left)
        left -= nb
        done += nb
        chain = recs[L * k:L * k + L]
        assert [r["kernel"] for r in chain] == list(chain_names)
        grids = [(r["gx"], r["gy"], r["gz"], r["block"]) for r in chain]
        lanes = nb * H * W * 3 // 4 + 1                                   # a lane per aligned dword of out and one for the ragged ends
        want = [(-(-lanes // 256), 1, 1, 256)]
        if style != "none":
            want = [(tiles, nb, 1, 256), (tiles, nb, 1, 256), (px, nb, 1, 256), (px, nb, 1, 256)] + want
            assert chain[0]["workspace"] == nb * (H * W * 4 + 16)          # the int32 label array and the whole-frame windows
        assert grids == want
        assert all(r["workspace"] == 0 for r in chain[1:]) and (style != "none" or chain[0]["workspace"] == 0)
        assert chain[-1]["writes"] == f"out={done * H * W * 3}"            # from the start of the caller's out
        assert all(r["writes"] == "-" for r in chain[:-1])
        for r in chain:
            assert r["lds"] == 0 and max(r["gy"], r["gz"]) <= gz_limit and r["gx"] < 1 << 31 and r["counters"] == 0
    assert left == 0 and recs[-1]["writes"] == f"out={B * H * W * 3}"
    cb = min(mb, B)
    assert ws == cb * (H * W * (ch + 1 + 3) + 16) + (cb * (H * W * 4 + 16) if style != "none" else 0)    # the header's MEMORY paragraph


def test_the_workspace_does_not_grow_with_the_video():
    for style in ("none", "fill"):
        a = OV.plan(128, 256, 256, 3, 128, style)[1]
        assert a == OV.plan(1280, 256, 256, 3, 128, style)[1] == OV.plan(129, 256, 256, 3, 128, style)[1]
        assert OV.plan(3, 256, 256, 3, 128, style)[1] < a                   # fewer frames than one micro-batch: what they need
        assert OV.plan(72, 480, 640, 3, 128, style)[1] == OV.plan(9999, 480, 640, 3, 128, style)[1]        # 64 MiB of out: 72 frames


def test_the_plan_refuses_what_the_entries_refuse():
    limit = lib().og_overlay_limit(0)
    out = C.create_string_buffer(1 << 16)
    for style in (-1, 3):
        assert lib().og_overlay_plan(1, 64, 64, 1, 32, style, out, len(out), None) == -1
    for args in ((0, 8, 8, 1, 32), (1, 0, 8, 1, 32), (1, 8, 8, 2, 32), (1, 8, 8, 1, 0), (1, 8, 8, 1, 1025), (1, 1, limit + 1, 1, 32)):
        with pytest.raises(OpenGlottalHipError):
            OV.plan(*args, style="fill")
    assert str(limit) in lib().og_last_error().decode()
    assert lib().og_overlay_plan(70, 300, 260, 1, 2, 2, out, 8, None) == -1 and b"does not fit" in lib().og_last_error()
    assert lib().og_overlay_plan(1, 8, 8, 1, 32, 2, None, 8, None) == -1
    recs, ws = OV.plan(1, 1, limit, 1, 1, "fill")                           # the largest frame, as one row
    assert recs[0]["gx"] == -(-limit // T) and ws == limit * 9 + 32
    with pytest.raises(OpenGlottalHipError):
        OV.plan(1, 8, 8, 1, 32, "solid")
