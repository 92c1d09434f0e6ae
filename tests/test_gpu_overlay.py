"""-m gpu: the overlay on the device (include/openglottal_hip_overlay.h) against its host twin, byte for byte: k_overlay and the
outside-background labelling through the tiled blob filter's launches, at the smallest frames at which they can go wrong -- one
tile and a bit, two tiles by one, a four-tile corner, one frame above the one-workgroup limit -- on every hard mask, three styles,
gray and BGR, every box case mixed with None in one launch, ragged micro-batches, a reused handle, and a prefilled out buffer."""
import numpy as np
import pytest

import classic_cases as K
import overlay_cases as OC
from openglottal_amd import overlay as OV
from openglottal_amd._lib import lib

pytestmark = pytest.mark.gpu

T = int(lib().og_classic_tiled_limit(1))
SHAPES = ((33, 33), (2 * T + 3, T + 5), (T + 1, 2 * T + 1), (2 * T + 1, 2 * T + 1))
_HOST = {}


def hard_batch(H, W):
    """Every hard mask at the side that covers the frame, cut to it; boxes: the cases in turn, None among them."""
    S = max(H, W)
    masks = np.stack([OC.cut(m, H, W) for _, m in K.hard_masks(S)])
    cases = OC.box_cases(H, W)
    boxes = np.array([cases[i % len(cases)][1] for i in range(len(masks))], np.int32)
    return masks, boxes


def host(frames, masks, boxes, style):
    """overlay_host frame by frame, computed once per input."""
    key = (frames.tobytes(), None if masks is None else masks.tobytes(), None if boxes is None else boxes.tobytes(), style)
    if key not in _HOST:
        _HOST[key] = np.stack([OV.overlay_host(frames[i], None if masks is None else masks[i], OC.ABSENT if boxes is None else boxes[i],
                                               style, normalized=True) for i in range(len(frames))])
    return _HOST[key]


def dev(e, frames, masks, boxes, style, fill=0xA5):
    import torch

    B, H, W = frames.shape[:3]
    ch = 3 if frames.ndim == 4 else 1
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    f, m, b = up(frames), up(masks), up(boxes)
    out = torch.full((B, H, W, 3), fill, dtype=torch.uint8, device="cuda")
    e.annotate_dev(f, B, H, W, ch, m, b, out, style)
    e.sync()
    return out.cpu().numpy()


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("H,W", SHAPES)
def test_device_equals_host_on_every_hard_mask(H, W, channels):
    masks, boxes = hard_batch(H, W)
    frames = OC.frames_for(len(masks), H, W, channels, seed=H + W)
    e = OV.Overlay(chunk=11)                                              # 28 masks: three micro-batches, the last ragged
    for style in OC.STYLES:
        want = host(frames, masks, boxes, style)
        for _ in range(2):                                                # each call made twice gives the same bits
            assert np.array_equal(dev(e, frames, masks, boxes, style), want), style
            assert np.array_equal(e.annotate(frames, masks, boxes, style), want), style
        assert np.array_equal(e.annotate(list(frames), masks, boxes, style), want), style
    # no boxes at all (every mask drawn, no rectangle), and no masks
    want = host(frames, masks, None, "fill")
    assert np.array_equal(dev(e, frames, masks, None, "fill"), want) and np.array_equal(e.annotate(frames, masks, None, "fill"), want)
    want = host(frames, None, boxes, "contour")
    assert np.array_equal(dev(e, frames, None, boxes, "contour"), want) and np.array_equal(e.annotate(frames, None, boxes, "contour"), want)


def seam_masks(H, W):
    """Holes and outside background that reach across a seam and across the four-tile corner at (T, T)."""
    out = []
    m = np.zeros((H, W), np.uint8)                                        # a ring around the corner: its hole spans four tiles
    m[T - 6:T + 7, T - 6:T + 7] = 255
    m[T - 3:T + 4, T - 3:T + 4] = 0
    m[T, T] = 255                                                         # an island in the hole, on the corner
    out.append(m)
    m = m.copy()                                                          # the hole opened to the outside through a one-pixel channel
    m[T - 1, T + 4:T + 7] = 0
    out.append(m)
    m = np.full((H, W), 255, np.uint8)                                    # a background snake that enters at the edge and crosses the seams
    m[T - 1, 0:T + 5] = 0
    m[T - 1:H - 2, T + 4] = 0
    m[H - 3, 3:T + 5] = 0
    out.append(m)
    m = m.copy()                                                          # the same snake cut off from the edge: one long hole
    m[T - 1, 0] = 255
    out.append(m)
    m = np.zeros((H, W), np.uint8)                                        # diagonal steps over the corner: 8-connected set, 4-connected ground
    for k in range(-8, 9):
        m[T + k, T + k] = 255
    out.append(m)
    m = np.zeros((H, W), np.uint8)                                        # a frame-sized ring: the whole interior is a hole
    m[0, :] = m[-1, :] = 255
    m[:, 0] = m[:, -1] = 255
    out.append(m)
    return np.stack(out)


def test_holes_and_outside_background_across_seams_and_a_four_tile_corner():
    H = W = 2 * T + 1
    masks = seam_masks(H, W)
    frames = OC.frames_for(len(masks), H, W, 3, seed=1)
    e = OV.Overlay()
    for style in ("contour", "fill"):
        want = host(frames, masks, None, style)
        assert np.array_equal(dev(e, frames, masks, None, style), want), style
    out = host(frames, masks, None, "contour")
    green = (out == (0, 255, 0)).all(-1)
    assert not green[0, T - 2:T + 3, T - 2:T + 3].any()                     # the closed hole and its island: no outline inside
    assert green[1, T - 4, T - 3] and not green[0, T - 4, T - 3]             # opened: the hole's border is outside border now
    assert green[2].sum() > green[3].sum() == 4 * (H - 1)                    # cut off from the edge the snake is a hole: the frame's edge alone


def test_one_frame_above_the_one_workgroup_limit():
    H, W = 300, 260
    assert H * W > lib().og_classic_limit(0)
    rs = np.random.RandomState(5)
    canvas = (rs.rand(H, W) < 0.55).astype(np.uint8)
    hard = dict(K.hard_masks(160))
    canvas[20:180, 30:190] |= hard["rings"]
    canvas[120:280, 80:240] ^= hard["spiral"]
    masks = (canvas * 255)[None]
    frames = OC.frames_for(1, H, W, 3, seed=2)
    boxes = np.array([(40, 30, W, H)], np.int32)
    e = OV.Overlay()
    for style in OC.STYLES:
        want = host(frames, masks, boxes, style)
        assert np.array_equal(dev(e, frames, masks, boxes, style), want) and np.array_equal(e.annotate(frames, masks, boxes, style), want)


def test_five_frames_at_chunk_two():
    H, W = 2 * T + 3, T + 5
    masks, boxes = hard_batch(H, W)
    masks, boxes = masks[[0, 4, 8, 12, 20]], boxes[[0, 1, 2, 3, 5]]
    for ch in (1, 3):
        frames = OC.frames_for(5, H, W, ch, seed=9)
        e = OV.Overlay(chunk=2)                                           # three micro-batches, the last one ragged
        assert len(OV.plan(5, H, W, ch, 2, "fill")[0]) == 15
        for style in OC.STYLES:
            want = host(frames, masks, boxes, style)
            assert np.array_equal(dev(e, frames, masks, boxes, style), want) and np.array_equal(e.annotate(frames, masks, boxes, style), want)
            assert np.array_equal(OV.Overlay(chunk=128).annotate(frames, masks, boxes, style), want)


def test_a_used_handle_equals_a_fresh_one():
    """Stale labels are never read: a large frame, then a small one, then None boxes, on ONE handle."""
    used = OV.Overlay(chunk=3)
    big = (np.random.RandomState(3).rand(1, 300, 260) < 0.5).astype(np.uint8) * 255
    fb = OC.frames_for(1, 300, 260, 3, seed=4)
    assert np.array_equal(dev(used, fb, big, None, "fill"), host(fb, big, None, "fill"))
    masks, boxes = hard_batch(33, 33)
    frames = OC.frames_for(len(masks), 33, 33, 1, seed=6)
    none = np.full_like(boxes, -1)
    for bx in (boxes, none, None):
        for style in ("fill", "contour"):
            fresh = OV.Overlay(chunk=3)
            got = dev(used, frames, masks, bx, style)
            assert np.array_equal(got, dev(fresh, frames, masks, bx, style)) and np.array_equal(got, host(frames, masks, bx, style))
            assert np.array_equal(used.annotate(frames, masks, bx, style), got)
    src = np.repeat(frames[..., None], 3, -1)
    assert np.array_equal(dev(used, frames, masks, none, "fill"), src)      # None on every frame: the source alone


@pytest.mark.parametrize("H,W,channels", [(33, 33, 1), (T + 1, 2 * T + 1, 3), (5, 7, 1), (1, 1, 3), (3, 1, 1)])
def test_every_byte_of_a_prefilled_out_is_written(H, W, channels):
    """H * W * 3 is odd here for most shapes: frame bases inside the batch fall on every residue modulo 4."""
    B = 5
    frames = np.full((B, H, W, 3) if channels == 3 else (B, H, W), 0xA5, np.uint8)      # a source equal to the prefill ...
    masks = np.zeros((B, H, W), np.uint8)
    e = OV.Overlay(chunk=2)
    for fill in (0xA5, 0x5A):                                             # ... must come out the same whatever the prefill was
        assert (dev(e, frames, masks, None, "fill", fill) == 0xA5).all()
        assert (dev(e, frames, None, None, "none", fill) == 0xA5).all()
    import torch

    frames = OC.frames_for(B, H, W, channels, seed=H * W)
    masks = ((np.random.RandomState(1).rand(B, H, W) < 0.5) * 255).astype(np.uint8)
    want = host(frames, masks, None, "fill")
    f, m = torch.from_numpy(frames).cuda(), torch.from_numpy(masks).cuda()
    for off in (0, 1, 2, 3):                                              # out at every byte alignment, guard bytes on both sides
        buf = torch.full((B * H * W * 3 + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        e.annotate_dev(f, B, H, W, channels, m, None, buf[4 + off:], "fill")
        e.sync()
        got = buf.cpu().numpy()
        assert np.array_equal(got[4 + off:4 + off + want.size].reshape(want.shape), want), off
        assert (got[:4 + off] == 0xA5).all() and (got[4 + off + want.size:] == 0xA5).all(), off
