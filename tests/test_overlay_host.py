"""The drawing rules of include/openglottal_hip_overlay.h on the host twins (og_outline_host, og_overlay_host: the inline functions
k_overlay calls, with a sequential labelling) against two independent statements: scipy's 4-connected background labelling
(tests/overlay_cases.py) and the points Moore border following visits (find_external of tests/golden/gen_golden_vft.py).  No GPU."""
import importlib.util
import os
import sys

import numpy as np
import pytest

import classic_cases as K
import overlay_cases as OC
from openglottal_amd import overlay as OV


def _generator():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_golden_vft.py")
    spec = importlib.util.spec_from_file_location("gen_golden_vft_overlay", path)
    mod = importlib.util.module_from_spec(spec)
    keep = list(sys.path)                  # importing it only extends sys.path: not for the suite
    spec.loader.exec_module(mod)
    sys.path[:] = keep
    return mod


G = _generator()


def contour_points(mask):
    """bool [H,W]: the union of the points of the external contours by Moore border following."""
    out = np.zeros(mask.shape, bool)
    for c in G.find_external(mask):
        p = c.reshape(-1, 2)
        out[p[:, 1], p[:, 0]] = True
    return out


def random_masks():
    """400 seeded masks, 1 to 23 pixels a side, densities 0.2 to 0.9, a third of them morphologically closed."""
    from scipy import ndimage

    rs = np.random.RandomState(2024)
    for k in range(400):
        h, w = rs.randint(1, 24), rs.randint(1, 24)
        m = rs.rand(h, w) < rs.uniform(0.2, 0.9)
        if k % 3 == 0:
            m = ndimage.binary_closing(m, structure=np.ones((3, 3), bool))
        yield f"random-{k}-{h}x{w}", m.astype(np.uint8)


def _check_outline(name, m):
    got = OV.outline_host(m)
    assert set(np.unique(got)) <= {0, 255}, name
    want = OC.outline(m)
    assert np.array_equal(got > 0, want), name
    assert np.array_equal(want, OC.outline_filled(m)), name
    assert np.array_equal(got > 0, contour_points(m)), name


def test_outline_on_the_named_masks():
    for name, m in K.named_masks():
        _check_outline(name, m)
        _check_outline(name + " x255", (m * 255).astype(np.uint8))


@pytest.mark.parametrize("S", (33, 65, 96))
def test_outline_on_the_hard_masks(S):
    names = set()
    for name, m in K.hard_masks(S):
        names.add(name)
        _check_outline(f"{name}-{S}", m)
    assert {"spiral", "serpentine-T", "rings-rot", "checkerboard-inv", "stairs"} <= names


def test_outline_on_400_random_masks():
    n = 0
    for name, m in random_masks():
        _check_outline(name, m)
        n += 1
    assert n == 400


def test_what_lies_inside_a_hole_gets_no_outline():
    m = np.zeros((15, 17), np.uint8)
    m[2:13, 3:14] = 1
    m[4:11, 5:12] = 0                      # a ring
    ring = OV.outline_host(m) > 0
    m[7, 8] = 1                            # an island inside the hole
    assert np.array_equal(OV.outline_host(m) > 0, ring) and not ring[7, 8]
    m[6:9, 7:10] = 1
    m[7, 8] = 0                            # a ring inside the ring
    assert np.array_equal(OV.outline_host(m) > 0, ring)
    want = np.zeros_like(ring)
    want[2, 3:14] = want[12, 3:14] = want[2:13, 3] = want[2:13, 13] = True
    assert np.array_equal(ring, want)      # the outer border only: the hole's inner border is not external


def test_a_full_mask_outlines_exactly_the_frames_edge():
    for h, w in ((1, 1), (1, 7), (6, 1), (2, 2), (9, 11), (33, 40)):
        got = OV.outline_host(np.full((h, w), 255, np.uint8)) > 0
        want = np.ones((h, w), bool)
        want[1:-1, 1:-1] = False
        assert np.array_equal(got, want), (h, w)


H, W = 24, 31


def _mask():
    m = np.zeros((H, W), np.uint8)
    m[3:20, 4:27] = 255
    m[7:15, 9:20] = 0
    m[10, 13] = 255
    m[0, 0] = m[H - 1, W - 1] = 255
    m[22, 2:9] = 7                         # any nonzero byte counts
    return m


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("style", OC.STYLES)
def test_overlay_host_equals_the_numpy_statement(style, channels):
    frames = OC.frames_for(4, H, W, channels, seed=3)
    m = _mask()
    cases = OC.box_cases(H, W) + [("no-boxes", OC.ABSENT)]
    for k, (name, box) in enumerate(cases):
        f = frames[k % len(frames)]
        for mask in (m, None):
            got = OV.overlay_host(f, mask, box, style, normalized=True)
            assert got.shape == (H, W, 3) and got.dtype == np.uint8
            assert np.array_equal(got, OC.overlay(f, mask, box, style)), (name, mask is None)
    # as the detector returns it: None, and a box whose far corner lies on x2 == W, y2 == H
    f = frames[3]
    assert np.array_equal(OV.overlay_host(f, m, None, style), OC.overlay(f, m, (-1, -1, -1, -1), style))
    assert np.array_equal(OV.overlay_host(f, m, (5, 6, W, H), style), OC.overlay(f, m, (5, 6, W, H), style))
    src = f if channels == 3 else np.repeat(f[:, :, None], 3, 2)
    assert np.array_equal(OV.overlay_host(f, m, None, style), src)           # None: neither mask nor rectangle


def test_the_fill_saturates_at_source_g_153():
    for g in range(256):
        f = np.zeros((3, 3, 3), np.uint8)
        f[..., 0], f[..., 1], f[..., 2] = 9, g, 200
        m = np.zeros((3, 3), np.uint8)
        m[1, 1] = 255                      # one pixel: it is its own outline ...
        out = OV.overlay_host(f, np.full((3, 3), 255, np.uint8), OC.ABSENT, "fill")
        assert tuple(out[1, 1]) == (9, min(255, g + 102), 200), g            # ... so take the interior of a full mask
        assert (min(255, g + 102) == 255) == (g >= 153)
        assert tuple(OV.overlay_host(f, m, OC.ABSENT, "fill")[1, 1]) == (0, 255, 0)
        assert tuple(OV.overlay_host(f, m, OC.ABSENT, "contour")[0, 0]) == (9, g, 200)
    gray = np.full((3, 3), 153, np.uint8)
    assert tuple(OV.overlay_host(gray, np.full((3, 3), 1, np.uint8), OC.ABSENT, "fill")[1, 1]) == (153, 255, 153)


def test_draw_order_mask_then_outline_then_rectangle():
    f = np.full((9, 9, 3), 50, np.uint8)
    m = np.zeros((9, 9), np.uint8)
    m[2:7, 2:7] = 255
    out = OV.overlay_host(f, m, (2, 2, 4, 4), "fill", normalized=True)
    assert tuple(out[2, 2]) == (0, 220, 255)                                 # mask, outline and rectangle: yellow
    assert tuple(out[6, 6]) == (0, 255, 0)                                   # mask and outline: green
    assert tuple(out[4, 3]) == (0, 220, 255)                                 # mask and rectangle
    assert tuple(out[5, 5]) == (50, 152, 50)                                 # mask alone: the fill
    assert tuple(out[0, 0]) == (50, 50, 50)
    assert tuple(OV.overlay_host(f, m, (2, 2, 4, 4), "none", normalized=True)[6, 6]) == (50, 50, 50)


def test_draw_overlay_returns_a_fresh_array_and_leaves_its_inputs():
    f = OC.frames_for(1, H, W, 3, seed=8)[0]
    m = _mask()
    f0, m0 = f.copy(), m.copy()
    box = (5, 6, 20, 18)
    out = OV.draw_overlay(f, m, box, 123.0)
    assert out is not f and not np.shares_memory(out, f) and out.flags.writeable
    assert np.array_equal(f, f0) and np.array_equal(m, m0) and box == (5, 6, 20, 18)
    assert np.array_equal(out, OC.overlay(f, m, box, "fill"))
    assert np.array_equal(OV.draw_overlay(f, m, box, 0, overlay_style="contour"), OC.overlay(f, m, box, "contour"))
    assert np.array_equal(OV.draw_overlay(f, m, None, 0), OC.overlay(f, m, OC.ABSENT, "fill"))      # _draw_overlay: the mask is still drawn
    assert np.array_equal(OV.draw_overlay(f, None, box, 0), OC.overlay(f, None, box, "fill"))
    with pytest.raises(OV.OpenGlottalHipError):
        OV.draw_overlay(f, m, box, 0, overlay_style="solid")
