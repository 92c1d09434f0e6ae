"""Annotated frames (include/openglottal_hip_overlay.h): what ``scripts/infer.py:91-124`` (``_draw_overlay``) burns into a frame --
the glottis mask as a translucent green fill and a one-pixel outline, the detector's box in yellow -- drawn on the device, plus the
host twins that run the same inline functions on the CPU.

``Overlay`` wraps one ``og_overlay`` handle: its stream and the workspace of one micro-batch.  Boxes are given as the detector
returns them (``(x1, y1, x2, y2)`` or ``None``) and go through ``utils.normalize_box`` before they reach the library.  The text
label is not drawn on the device (its glyphs are OpenCV's Hershey table); ``label_host`` draws one with Pillow's built-in font.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import OpenGlottalHipError, check, lib, ptr
from .classic import _frames, boxes_array
from .utils import normalize_box

STYLES = {"none": 0, "contour": 1, "fill": 2}


def _style(style) -> int:
    if style not in STYLES:
        raise OpenGlottalHipError(f"overlay style must be one of {sorted(STYLES)}, got {style!r}")
    return STYLES[style]


def _masks(masks, B: int, H: int, W: int):
    if masks is None:
        return None
    m = np.ascontiguousarray(masks, dtype=np.uint8)
    if m.shape != (B, H, W):
        raise OpenGlottalHipError(f"expected masks of shape {(B, H, W)}, got {m.shape}")
    return m


class Overlay:
    """One ``og_overlay`` handle.  The device is the current one at the first call that touches it."""

    def __init__(self, chunk: int = 128):
        self._h = lib().og_overlay_create()
        if not self._h:
            raise OpenGlottalHipError("og_overlay_create failed")
        self.set_chunk(chunk)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().og_overlay_destroy(h)
            except Exception:
                pass

    def set_chunk(self, chunk: int) -> None:
        check(lib().og_overlay_set_chunk(self._h, int(chunk)), "og_overlay_set_chunk")
        self.chunk = int(chunk)

    def sync(self) -> None:
        check(lib().og_overlay_sync(self._h), "og_overlay_sync")

    def annotate(self, frames, masks, boxes, style: str = "fill") -> np.ndarray:
        """Host in, host out: frames ``[B,H,W]`` / ``[B,H,W,3]`` u8 (an array or a list), masks ``[B,H,W]`` u8 or ``None``, boxes a
        list of ``(x1, y1, x2, y2)`` / ``None`` per frame or ``None`` for no boxes at all.  Returns ``[B,H,W,3]`` u8."""
        arr, keep, B, H, W, ch = _frames(frames)
        m = _masks(masks, B, H, W)
        bx = None if boxes is None else boxes_array(boxes, B, W, H)
        out = np.empty((B, H, W, 3), np.uint8)
        if B:
            if keep is not None:
                ptrs = (C.c_void_p * B)(*[k.ctypes.data for k in keep])
                check(lib().og_overlay_stream_frames_u8(self._h, ptrs, B, H, W, ch, ptr(m), ptr(bx), _style(style), ptr(out)),
                      "og_overlay_stream_frames_u8")
            else:
                check(lib().og_overlay_stream_u8(self._h, ptr(arr), B, H, W, ch, ptr(m), ptr(bx), _style(style), ptr(out)),
                      "og_overlay_stream_u8")
        return out

    def annotate_dev(self, frames_dev, B: int, H: int, W: int, channels: int, masks_dev, boxes_dev, out_dev, style: str = "fill") -> None:
        """Resident, asynchronous variant (torch CUDA tensors or raw ints; ``masks_dev`` and ``boxes_dev`` may be ``None``)."""
        check(lib().og_overlay_u8_dev(self._h, ptr(frames_dev), B, H, W, channels, ptr(masks_dev), ptr(boxes_dev), _style(style),
                                      ptr(out_dev)), "og_overlay_u8_dev")


# ── host twins: the same inline functions on the CPU, no device ───────────────────────────────────────────────────────
def outline_host(mask) -> np.ndarray:
    """The one-pixel outline of the external contours of ``mask`` ``[H,W]`` (nonzero = set): u8 {0, 255}."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    H, W = m.shape
    out = np.empty((H, W), np.uint8)
    check(lib().og_outline_host(ptr(m), H, W, ptr(out)), "og_outline_host")
    return out


def overlay_host(frame, mask, box, style: str = "fill", normalized: bool = False) -> np.ndarray:
    """One frame ``[H,W]`` / ``[H,W,3]`` u8 -> ``[H,W,3]`` u8.  ``box``: as the detector returns it, ``None`` for a frame without
    one, or the string ``"absent"`` for a call without boxes at all (the ``unet-only`` pipeline: the mask is drawn, no rectangle).
    ``normalized``: ``box`` is already a ``normalize_box`` row."""
    f = np.ascontiguousarray(frame, dtype=np.uint8)
    H, W = f.shape[:2]
    ch = 3 if f.ndim == 3 else 1
    if f.ndim == 3 and f.shape[2] != 3:
        raise OpenGlottalHipError(f"expected [H,W] or [H,W,3], got {f.shape}")
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
    if m is not None and m.shape != (H, W):
        raise OpenGlottalHipError(f"expected a mask of shape {(H, W)}, got {m.shape}")
    if isinstance(box, str):
        if box != "absent":
            raise OpenGlottalHipError(f"box must be a box, None or 'absent', got {box!r}")
        b = None
    else:
        b = np.array(box if normalized else normalize_box(box, W, H), np.int32)
    out = np.empty((H, W, 3), np.uint8)
    check(lib().og_overlay_host(ptr(f), H, W, ch, ptr(m), ptr(b), _style(style), ptr(out)), "og_overlay_host")
    return out


def draw_overlay(frame_bgr, mask, box, area, overlay_style: str = "fill", label: bool = False) -> np.ndarray:
    """``_draw_overlay`` for one frame, through ``og_overlay_host``: a fresh array, the inputs untouched, the same bits as the device
    pass.  As there, ``box is None`` draws no rectangle and the mask is still drawn.  ``area`` feeds only the optional host label."""
    out = overlay_host(frame_bgr, mask, "absent" if box is None else box, overlay_style)
    return label_host(out, area) if label else out


def label_host(frame_bgr, area) -> np.ndarray:
    """``area=N`` in white at (4, 14) with Pillow's built-in font -- NOT OpenCV's Hershey glyphs, so no pixel of it is pinned."""
    from PIL import Image, ImageDraw, ImageFont

    img = Image.fromarray(np.ascontiguousarray(frame_bgr, dtype=np.uint8))
    font = ImageFont.load_default()
    text = f"area={int(area)}"
    box = ImageDraw.Draw(img).textbbox((0, 0), text, font=font)
    ImageDraw.Draw(img).text((4, 14 - (box[3] - box[1])), text, fill=(255, 255, 255), font=font)   # (4, 14) is the baseline's left end
    return np.asarray(img).copy()


def plan(B: int, H: int, W: int, channels: int, chunk: int = 128, style: str = "fill"):
    """Dry run of the streamed pass: ``(records, workspace_bytes)``; a record is a dict of the plan line's fields."""
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong()
    n = lib().og_overlay_plan(B, H, W, channels, chunk, _style(style), out, len(out), C.byref(ws))
    if n < 0:
        check(n, "og_overlay_plan")
    names = ("kernel", "gx", "gy", "gz", "block", "lds", "workspace", "counters", "writes")
    recs = []
    for line in out.value.decode().splitlines():
        parts = line.split("|")
        recs.append({k: (v if k in ("kernel", "writes") else int(v)) for k, v in zip(names, parts)})
    assert len(recs) == n
    return recs, ws.value
