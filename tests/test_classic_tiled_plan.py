"""og_classic_plan_tiled: the launches, grids and workspace of the streamed guided-VFT pass with the tiled blob filter, walked without a
GPU.  Tile kernels run on (tiles of the frame, frames of the micro-batch), per-pixel kernels on (ceil(pixels / 256), frames), the
selection on one workgroup per frame; the kernel names are a closed set; mode 1 up to 65 536 pixels is og_classic_plan's text."""
import ctypes as C

import pytest

from openglottal_amd import classic as CL
from openglottal_amd._lib import OpenGlottalHipError, lib

MiB = 1 << 20
T = int(lib().og_classic_tiled_limit(1))

# the launches of one micro-batch in tiled mode, in order ({ch}: the channel count of the source frames)
TILED_CHAIN = ("k_box_hist<{ch}>", "k_vft_thresholds", "k_tblob_background<{ch}>", "k_tblob_seams<false>", "k_tblob_flatten", "k_tblob_border",
               "k_tblob_fill", "k_tblob_seams<true>", "k_tblob_flatten", "k_tblob_keys", "k_tblob_select", "k_tblob_paint")
UNTILED_CHAIN = ("k_box_hist<{ch}>", "k_vft_thresholds", "k_blobs<{ch}>")
CLOSED = {k.format(ch=ch) for k in TILED_CHAIN + UNTILED_CHAIN for ch in (1, 3)}


def micro_batch(chunk, H, W, ch):
    return max(1, min(chunk, (64 * MiB) // (H * W * ch)))


def text(fn, *args):
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong()
    n = fn(*args, out, len(out), C.byref(ws))
    assert n > 0
    return out.value.decode(), ws.value


@pytest.mark.parametrize("B,H,W,ch,chunk", [(1, 256, 256, 1, 32), (70, 256, 256, 3, 32), (5, 17, 23, 1, 2), (9, 120, 160, 3, 32)])
def test_auto_up_to_the_old_limit_is_the_untiled_plan(B, H, W, ch, chunk):
    assert text(lib().og_classic_plan_tiled, B, H, W, ch, chunk, 1) == text(lib().og_classic_plan, B, H, W, ch, chunk)
    assert CL.plan(B, H, W, ch, chunk, tiled="auto") == CL.plan(B, H, W, ch, chunk)
    assert {r["kernel"] for r in CL.plan(B, H, W, ch, chunk, tiled="auto")[0]} == {k.format(ch=ch) for k in UNTILED_CHAIN}


@pytest.mark.parametrize("mode,B,H,W,ch,chunk", [("always", 5, 2 * T + 3, T + 5, 1, 2), ("always", 3, 2 * T + 3, T + 5, 3, 32),
                                                 ("auto", 100, 480, 640, 3, 128), ("auto", 3, 480, 640, 1, 128),
                                                 ("auto", 25, 1080, 1920, 3, 128), ("always", 7, 256, 256, 3, 4)])
def test_tiled_plan_lists_each_kernel_with_its_grid(mode, B, H, W, ch, chunk):
    recs, ws = CL.plan(B, H, W, ch, chunk, tiled=mode)
    mb = micro_batch(chunk, H, W, ch)
    n_batches = -(-B // mb)
    L = len(TILED_CHAIN)
    assert len(recs) == L * n_batches
    gz_limit = lib().og_workspace_limit(2)
    tiles = -(-H // T) * -(-W // T)
    px = -(-(H * W) // 256)
    hist = 4 * -(-(H * W) // 65536) if H * W > 65536 else 4              # four blocks per 65 536 pixels of the frame
    left = B
    for k in range(n_batches):
        nb = min(mb, left)
        left -= nb
        chain = recs[L * k:L * k + L]
        assert [r["kernel"] for r in chain] == [name.format(ch=ch) for name in TILED_CHAIN]
        grids = [(r["gx"], r["gy"], r["gz"], r["block"]) for r in chain]
        assert grids == [(hist, nb, 1, 256), (1, 1, 1, 256),
                         (tiles, nb, 1, 256), (tiles, nb, 1, 256), (px, nb, 1, 256), (px, nb, 1, 256),
                         (tiles, nb, 1, 256), (tiles, nb, 1, 256), (px, nb, 1, 256), (-(-((H + 1) * (W + 1)) // 256), nb, 1, 256),
                         (nb, 1, 1, 1024), (px, nb, 1, 256)]
        assert chain[2]["workspace"] == nb * (H * W * 8 + 36)              # two int32 label arrays and the roots taken, per frame
        assert all(r["workspace"] == 0 for i, r in enumerate(chain) if i != 2)
        assert chain[-1]["writes"] == f"mask={nb * H * W};area={4 * nb}"   # inside the micro-batch's buffers
        assert all(r["writes"] == "-" for r in chain[:-1])
        for r in chain:
            assert r["lds"] == 0 and max(r["gy"], r["gz"]) <= gz_limit and r["gx"] < 1 << 31 and r["counters"] == 0
    assert left == 0
    cb = min(mb, B)
    assert ws == cb * (H * W * (ch + 1 + 8) + 1096) + 8                    # the header's MEMORY paragraph
    assert {r["kernel"] for r in recs} <= CLOSED


def test_the_kernel_names_are_a_closed_set():
    seen = set()
    for mode in ("off", "auto", "always"):
        for (H, W) in ((64, 64), (256, 256), (300, 260), (480, 640)):
            if mode == "off" and H * W > 65536:
                continue
            for ch in (1, 3):
                seen |= {r["kernel"] for r in CL.plan(3, H, W, ch, 2, tiled=mode)[0]}
    assert seen == CLOSED


def test_the_tiled_plan_refuses_what_the_entries_refuse():
    limit = lib().og_classic_tiled_limit(0)
    out = C.create_string_buffer(1 << 16)
    for mode in (0, 3, -1):
        assert lib().og_classic_plan_tiled(1, 64, 64, 1, 32, mode, out, len(out), None) == -1
    for args in ((0, 8, 8, 1, 32), (1, 0, 8, 1, 32), (1, 8, 8, 2, 32), (1, 8, 8, 1, 0), (1, 8, 8, 1, 1025), (1, 1, limit + 1, 1, 32)):
        for mode in ("auto", "always"):
            with pytest.raises(OpenGlottalHipError):
                CL.plan(*args, tiled=mode)
    assert str(limit) in lib().og_last_error().decode()
    assert lib().og_classic_plan_tiled(70, 300, 260, 1, 32, 1, out, 8, None) == -1 and b"does not fit" in lib().og_last_error()
    with pytest.raises(OpenGlottalHipError):
        CL.plan(1, 257, 256, 1, 32)                                       # the untiled plan keeps its limit
    recs, ws = CL.plan(1, 1, limit, 1, 1, tiled="auto")                   # the largest frame, as one row
    assert recs[2]["gx"] == -(-limit // T) and ws == limit * 10 + 1096 + 8
