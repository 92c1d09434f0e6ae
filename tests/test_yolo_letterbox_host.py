"""CPU: the detector's device letterbox, checked where no device is needed.

``openglottal_amd.yolo.letterbox_bgr`` (ultralytics ``LetterBox(auto=True, stride=32)`` over ``geometry.resize_linear``) is the
specification.  ``og_yolo_letterbox_geometry`` restates its scalars and ``og_yolo_letterbox_host`` loops the very inline function
``k_letterbox_bgr`` calls per pixel, so every tap, coefficient and pad byte is held to the specification here, on noise.
"""
import ctypes as C

import numpy as np
import pytest

from openglottal_amd._lib import lib
from openglottal_amd.yolo import letterbox_bgr

OG_EINVAL = -1

# source H, W -> network H, W (computed with letterbox_bgr; asserted below)
SHAPES = {
    (480, 640): (192, 256),   # no pad
    (640, 480): (256, 192),   # portrait
    (360, 640): (160, 256),   # pad_top 8
    (299, 500): (160, 256),   # odd pad: top 3, bottom 4
    (500, 299): (256, 160),   # its transpose
    (100, 120): (224, 256),   # gain 2.13, upscale, top 5 / bottom 6
    (128, 128): (256, 256),   # gain 2
    (256, 512): (128, 256),   # exact 2x down
    (33, 700): (32, 256),     # 12 content rows, pads 10 / 10
    (250, 250): (256, 256),   # gain 1.024, no pad
    (224, 256): (224, 256),   # identity
    (256, 256): (256, 256),   # identity
}


def c_geometry(h, w, imgsz):
    i = [C.c_int() for _ in range(6)]
    g = C.c_double()
    rc = lib().og_yolo_letterbox_geometry(h, w, imgsz, *[C.byref(v) for v in i], C.byref(g))
    return rc, tuple(v.value for v in i), g.value


def py_geometry(h, w, imgsz, stride=32):
    """letterbox_bgr's scalars, restated: (net_h, net_w, new_h, new_w, pad_top, pad_left), gain; None where a side rounds to 0."""
    r = min(imgsz / h, imgsz / w)
    nw, nh = int(round(w * r)), int(round(h * r))
    if nw < 1 or nh < 1:
        return None
    dw, dh = (imgsz - nw) % stride, (imgsz - nh) % stride
    top, left = int(round(dh / 2 - 0.1)), int(round(dw / 2 - 0.1))
    bottom, right = int(round(dh / 2 + 0.1)), int(round(dw / 2 + 0.1))
    return (nh + top + bottom, nw + left + right, nh, nw, top, left), r


def test_c1_geometry_equals_the_python_scalars_everywhere():
    special = (1, 2, 3, 5, 31, 32, 33, 255, 256, 257, 511, 512, 513, 700, 1080, 1920, 8192)
    pairs = [(h, w) for h in range(1, 301) for w in range(1, 301)] + [(h, w) for h in special for w in special]
    n_bad = 0
    for imgsz in (256, 640):
        for h, w in pairs:
            rc, ints, gain = c_geometry(h, w, imgsz)
            ref = py_geometry(h, w, imgsz)
            if ref is None:
                n_bad += 1
                assert rc == OG_EINVAL, (h, w, imgsz)
            else:
                assert rc == 0 and ints == ref[0] and gain == ref[1], (h, w, imgsz, ints, gain, ref)
    assert n_bad > 0 and c_geometry(1, 700, 256)[0] == OG_EINVAL          # a rounded side of 0 occurs in the sweep
    for h, w, imgsz in ((0, 5, 256), (5, 0, 256), (-1, 5, 256), (8193, 5, 256), (5, 8193, 256), (5, 5, 0), (5, 5, -32), (5, 5, 250),
                        (5, 5, 16), (5, 5, 257)):
        assert c_geometry(h, w, imgsz)[0] == OG_EINVAL, (h, w, imgsz)
    assert c_geometry(8192, 8192, 256)[0] == 0


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_c1_geometry_equals_letterbox_bgr_on_the_shapes(shape):
    h, w = shape
    img, gain, left, top = letterbox_bgr(np.zeros((h, w, 3), np.uint8), 256)
    rc, (net_h, net_w, new_h, new_w, pad_top, pad_left), g = c_geometry(h, w, 256)
    assert rc == 0
    assert (net_h, net_w) == img.shape[:2] == SHAPES[shape]
    assert (g, pad_left, pad_top) == (gain, left, top)
    assert (new_h, new_w) == (int(round(h * gain)), int(round(w * gain)))


def c_letterbox(frame, imgsz=256):
    h, w = frame.shape[:2]
    ch = 1 if frame.ndim == 2 else frame.shape[2]
    rc, ints, _ = c_geometry(h, w, imgsz)
    assert rc == 0
    out = np.full((ints[0], ints[1], 3), 7, np.uint8)
    f = np.ascontiguousarray(frame)
    assert lib().og_yolo_letterbox_host(f.ctypes.data, h, w, ch, imgsz, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_c2_host_letterbox_equals_letterbox_bgr_byte_for_byte(shape):
    h, w = shape
    rs = np.random.RandomState(h * 1000 + w)
    bgr = rs.randint(0, 256, (h, w, 3), dtype=np.uint8)
    ref = letterbox_bgr(bgr, 256)[0]
    assert np.array_equal(c_letterbox(bgr), ref)
    gray = rs.randint(0, 256, (h, w), dtype=np.uint8)
    ref1 = letterbox_bgr(np.repeat(gray[..., None], 3, axis=-1), 256)[0]
    assert np.array_equal(c_letterbox(gray), ref1)
    if SHAPES[shape] == shape:                                                # identity: the output is the input
        assert np.array_equal(c_letterbox(bgr), bgr)
        assert np.array_equal(c_letterbox(gray), np.repeat(gray[..., None], 3, axis=-1))


def test_c2_the_rule_is_a_copy_at_equal_size_for_every_byte_value():
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 256).repeat(32, axis=0)   # 32 x 256: identity geometry, every s in 0..255
    assert np.array_equal(c_letterbox(ramp)[..., 1], ramp)


def test_c3_argument_errors_on_a_handle():
    h = lib().og_yolo_create(1)
    assert h
    try:
        buf = np.zeros(64 * 64 * 3, np.uint8)
        best = np.zeros(5, np.float32)
        p, q = buf.ctypes.data, best.ctypes.data
        for channels, imgsz in ((2, 256), (0, 256), (4, 256), (3, 250), (3, 0), (3, -32)):
            assert lib().og_yolo_detect_resized_u8(h, p, 1, 64, 64, channels, imgsz, 0.25, q) == OG_EINVAL, (channels, imgsz)
            assert lib().og_yolo_detect_resized_u8_dev(h, p, 1, 64, 64, channels, imgsz, 0.25, q) == OG_EINVAL, (channels, imgsz)
            assert lib().og_yolo_detect_resized_u8_begin(h, p, 1, 64, 64, channels, imgsz, 0.25) == OG_EINVAL, (channels, imgsz)
            assert lib().og_yolo_letterbox_u8_dev(h, p, 1, 64, 64, channels, imgsz, p) == OG_EINVAL, (channels, imgsz)
        assert lib().og_yolo_letterbox_host(p, 64, 64, 2, 256, p) == OG_EINVAL
        assert lib().og_yolo_letterbox_host(p, 64, 64, 3, 250, p) == OG_EINVAL
        assert lib().og_yolo_detect_resized_u8(h, p, 1, 1, 700, 3, 256, 0.25, q) == OG_EINVAL      # a content side of 0
        for v in (0, -1):
            assert lib().og_yolo_set_option(h, b"source_stage_kib", v) == OG_EINVAL, v
        assert lib().og_yolo_set_option(h, b"source_stage_kib", 1) == 0
        assert lib().og_yolo_set_option(h, b"source_stage_kib", 65536) == 0
        assert lib().og_yolo_launch_count(h, b"k_letterbox_bgr") == 0 and lib().og_yolo_launch_count(h, b"k_scale_boxes") == 0
        assert lib().og_yolo_launch_count(h, b"k_conv") == OG_EINVAL
    finally:
        lib().og_yolo_destroy(h)
