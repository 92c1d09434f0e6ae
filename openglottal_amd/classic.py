"""The training-free family on the device (include/openglottal_hip_classic.h): guided-VFT (`openglottal/models/tracker.py:117-232`)
and YOLO+Otsu (`scripts/eval_girafe.py:162-171`), plus the host twins that run the same inline functions on the CPU.

``Classic`` wraps one ``og_classic`` handle: its stream, the workspace of one micro-batch and the running threshold of the
guided-VFT recurrence.  Boxes are given as the detector returns them (``(x1, y1, x2, y2)`` or ``None``) and go through
``utils.normalize_box`` -- the Python slice semantics of ``m[y1:y2, x1:x2] = 255`` -- before they reach the library.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import OpenGlottalHipError, check, lib, ptr
from .utils import normalize_box


def _frames(frames):
    """-> (array | None, list | None, B, H, W, channels) for ``[B,H,W]`` / ``[B,H,W,3]`` u8 frames given as an array or a list."""
    keep = arr = None
    if isinstance(frames, (list, tuple)):
        keep = [f if (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.flags.c_contiguous) else np.ascontiguousarray(f, dtype=np.uint8)
                for f in frames]
        if keep and any(f.shape != keep[0].shape for f in keep):
            raise OpenGlottalHipError("frames of a list must share one [H,W] or [H,W,3] shape")
        shape = (len(keep),) + (keep[0].shape if keep else (0, 0))
    else:
        arr = np.ascontiguousarray(frames, dtype=np.uint8)
        shape = arr.shape
    if len(shape) == 4 and shape[-1] == 3:
        ch = 3
    elif len(shape) == 3:
        ch = 1
    else:
        raise OpenGlottalHipError(f"expected [B,H,W] or [B,H,W,3] frames, got {shape}")
    return arr, keep, int(shape[0]), int(shape[1]), int(shape[2]), ch


def boxes_array(boxes, B: int, W: int, H: int) -> np.ndarray:
    """``[B,4]`` int32 of ``normalize_box`` rows (an int32 ``[B,4]`` array is taken as already normalised)."""
    if isinstance(boxes, np.ndarray) and boxes.dtype == np.int32 and boxes.shape == (B, 4):
        return np.ascontiguousarray(boxes)
    if len(boxes) != B:
        raise OpenGlottalHipError(f"{len(boxes)} boxes for {B} frames")
    return np.array([normalize_box(b, W, H) for b in boxes], np.int32).reshape(B, 4)


TILED_MODES = {"off": 0, "auto": 1, "always": 2}


def _tiled_mode(tiled) -> int:
    if tiled not in TILED_MODES:
        raise OpenGlottalHipError(f"tiled must be one of {sorted(TILED_MODES)}, got {tiled!r}")
    return TILED_MODES[tiled]


class Classic:
    """One ``og_classic`` handle.  The device is the current one at the first call that touches it.  ``tiled``
    (include/openglottal_hip_classic_tiled.h): ``"off"`` keeps the one-workgroup blob filter and its 65 536-pixel limit, ``"auto"``
    takes the tiled filter above that size, ``"always"`` at every size."""

    def __init__(self, beta: float = 0.7, percentile: float = 30, n_components: int = 2, chunk: int = 128, tiled: str = "off"):
        self._h = lib().og_classic_create()
        if not self._h:
            raise OpenGlottalHipError("og_classic_create failed")
        self.reset(beta, percentile, n_components)
        self.set_chunk(chunk)
        self.set_tiled(tiled)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().og_classic_destroy(h)
            except Exception:
                pass

    def reset(self, beta: float, percentile: float, n_components: int) -> None:
        check(lib().og_vft_guided_reset(self._h, float(beta), float(percentile), int(n_components)), "og_vft_guided_reset")

    def set_chunk(self, chunk: int) -> None:
        check(lib().og_classic_set_chunk(self._h, int(chunk)), "og_classic_set_chunk")
        self.chunk = int(chunk)

    def set_tiled(self, tiled: str) -> None:
        check(lib().og_classic_set_tiled(self._h, _tiled_mode(tiled)), "og_classic_set_tiled")
        self.tiled = tiled

    def sync(self) -> None:
        check(lib().og_classic_sync(self._h), "og_classic_sync")

    @property
    def thresh(self) -> float:
        t = C.c_double()
        check(lib().og_vft_guided_get_state(self._h, C.byref(t)), "og_vft_guided_get_state")
        return t.value

    @thresh.setter
    def thresh(self, value: float) -> None:
        check(lib().og_vft_guided_set_state(self._h, float(value)), "og_vft_guided_set_state")

    def init(self, frames, bbox=None) -> float:
        """``YOLOGuidedVFT.initialize``: seeds the threshold from the last frame inside ``bbox`` (whole frame when it is ``None`` or
        empty) and returns it."""
        arr, keep, n, H, W, ch = _frames(frames)
        if n < 1:
            raise OpenGlottalHipError("initialize needs at least one frame")
        last = np.ascontiguousarray(keep[-1] if keep is not None else arr[-1])
        box = None if bbox is None else np.array(normalize_box(bbox, W, H), np.int32)
        t = C.c_double()
        check(lib().og_vft_guided_init_u8(self._h, ptr(last), 1, H, W, ch, ptr(box), C.byref(t)), "og_vft_guided_init_u8")
        return t.value

    def guided_vft(self, frames, boxes, want_mask: bool = True, want_thresh: bool = False):
        """``process_frame`` over the frames in order, from the running threshold.  Returns ``(mask [B,H,W] u8 | None, area int32
        [B])`` and, with ``want_thresh``, the f64 threshold after each frame as a third element."""
        arr, keep, B, H, W, ch = _frames(frames)
        bx = boxes_array(boxes, B, W, H)
        mask = np.empty((B, H, W), np.uint8) if want_mask else None
        area = np.zeros(B, np.int32)
        th = np.zeros(B, np.float64) if want_thresh else None
        if B:
            if keep is not None:
                ptrs = (C.c_void_p * B)(*[k.ctypes.data for k in keep])
                check(lib().og_vft_guided_stream_frames_u8(self._h, ptrs, B, H, W, ch, ptr(bx), ptr(mask), ptr(area), ptr(th)),
                      "og_vft_guided_stream_frames_u8")
            else:
                check(lib().og_vft_guided_stream_u8(self._h, ptr(arr), B, H, W, ch, ptr(bx), ptr(mask), ptr(area), ptr(th)),
                      "og_vft_guided_stream_u8")
        return (mask, area, th) if want_thresh else (mask, area)

    def guided_vft_dev(self, frames_dev, B: int, H: int, W: int, channels: int, boxes_dev, area_dev, mask_dev=None, thresh_dev=None) -> None:
        """Resident, asynchronous variant (torch CUDA tensors or raw ints)."""
        check(lib().og_vft_guided_u8_dev(self._h, ptr(frames_dev), B, H, W, channels, ptr(boxes_dev), ptr(mask_dev), ptr(area_dev),
                                         ptr(thresh_dev)), "og_vft_guided_u8_dev")

    def otsu_in_box(self, frames, boxes, want_mask: bool = True):
        """``yolo+otsu``: ``(mask [B,H,W] u8 | None, area int32 [B], T int32 [B])``."""
        arr, keep, B, H, W, ch = _frames(frames)
        if keep is not None:
            arr = np.stack(keep) if keep else np.zeros((0, H, W), np.uint8)
        bx = boxes_array(boxes, B, W, H)
        mask = np.empty((B, H, W), np.uint8) if want_mask else None
        area = np.zeros(B, np.int32)
        T = np.zeros(B, np.int32)
        if B:
            check(lib().og_otsu_in_box_u8(self._h, ptr(arr), B, H, W, ch, ptr(bx), ptr(mask), ptr(area), ptr(T)), "og_otsu_in_box_u8")
        return mask, area, T

    def otsu_in_box_dev(self, frames_dev, B: int, H: int, W: int, channels: int, boxes_dev, area_dev, T_dev, mask_dev=None) -> None:
        check(lib().og_otsu_in_box_u8_dev(self._h, ptr(frames_dev), B, H, W, channels, ptr(boxes_dev), ptr(mask_dev), ptr(area_dev),
                                          ptr(T_dev)), "og_otsu_in_box_u8_dev")


# ── host twins: the same inline functions on the CPU, no device ───────────────────────────────────────────────────────
def percentile_host(hist256, q: float) -> float:
    h = np.ascontiguousarray(hist256, dtype=np.uint32)
    out = C.c_double()
    check(lib().og_percentile_host(ptr(h), float(q), C.byref(out)), "og_percentile_host")
    return out.value


def otsu_threshold_host(hist256) -> int:
    h = np.ascontiguousarray(hist256, dtype=np.uint32)
    T = C.c_int32()
    check(lib().og_otsu_threshold_host(ptr(h), C.byref(T)), "og_otsu_threshold_host")
    return T.value


def box_hist_host(frame, box) -> np.ndarray:
    """Histogram of the gray bytes of one ``[H,W]`` / ``[H,W,3]`` u8 frame inside ``box`` (as the detector returns it)."""
    f = np.ascontiguousarray(frame, dtype=np.uint8)
    H, W = f.shape[:2]
    b = np.array(normalize_box(box, W, H), np.int32)
    h = np.zeros(256, np.uint32)
    check(lib().og_box_hist_host(ptr(f), H, W, 3 if f.ndim == 3 else 1, ptr(b), ptr(h)), "og_box_hist_host")
    return h


def vft_step_host(thresh: float, beta: float, hist256, q: float):
    """One frame of the recurrence -> ``(thresh, cut)``."""
    h = np.ascontiguousarray(hist256, dtype=np.uint32)
    t, c = C.c_double(), C.c_int32()
    check(lib().og_vft_step_host(float(thresh), float(beta), ptr(h), float(q), C.byref(t), C.byref(c)), "og_vft_step_host")
    return t.value, c.value


def blobs_host(mask, n: int, want_mask: bool = True):
    """``_nblobs(mask, n)`` -> ``(mask u8 {0,255} | None, area)``."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    H, W = m.shape
    out = np.empty((H, W), np.uint8) if want_mask else None
    area = C.c_int32()
    if H * W > lib().og_classic_limit(0):
        check(lib().og_blobs_host_any(ptr(m), H, W, int(n), ptr(out), C.byref(area)), "og_blobs_host_any")
    else:
        check(lib().og_blobs_host(ptr(m), H, W, int(n), ptr(out), C.byref(area)), "og_blobs_host")
    return out, area.value


def guided_vft_host(frames, boxes, thresh: float, beta: float = 0.7, percentile: float = 30, n_components: int = 2):
    """The host composition of the guided-VFT pass, frame by frame: ``(masks, areas, threshs, final thresh)``.  A BGR frame is
    converted by ``utils.bgr_to_gray`` (one pass of ``og_bgr2gray_host`` for a contiguous u8 frame)."""
    from .utils import bgr_to_gray

    masks, areas, ths = [], [], []
    for f, b in zip(frames, boxes):
        f = np.asarray(f)
        H, W = f.shape[:2]
        thresh, cut = vft_step_host(thresh, beta, box_hist_host(f, b), percentile)
        g = bgr_to_gray(f) if f.ndim == 3 else f
        x1, y1, x2, y2 = normalize_box(b, W, H)
        raw = np.zeros((H, W), np.uint8)
        if x1 >= 0:
            raw[y1:y2, x1:x2] = (g[y1:y2, x1:x2].astype(np.int32) < cut) * 255
        m, a = blobs_host(raw, n_components)
        masks.append(m)
        areas.append(a)
        ths.append(thresh)
    return masks, np.array(areas, np.int32), np.array(ths, np.float64), thresh


def plan(B: int, H: int, W: int, channels: int, chunk: int = 128, tiled: str = "off"):
    """Dry run of the streamed guided-VFT pass: ``(records, workspace_bytes)``; a record is a dict of the plan line's fields."""
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong()
    mode = _tiled_mode(tiled)
    if mode:
        n = lib().og_classic_plan_tiled(B, H, W, channels, chunk, mode, out, len(out), C.byref(ws))
    else:
        n = lib().og_classic_plan(B, H, W, channels, chunk, out, len(out), C.byref(ws))
    if n < 0:
        check(n, "og_classic_plan_tiled" if mode else "og_classic_plan")
    names = ("kernel", "gx", "gy", "gz", "block", "lds", "workspace", "counters", "writes")
    recs = []
    for line in out.value.decode().splitlines():
        parts = line.split("|")
        recs.append({k: (v if k in ("kernel", "writes") else int(v)) for k, v in zip(names, parts)})
    assert len(recs) == n
    return recs, ws.value
