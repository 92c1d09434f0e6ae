"""The detection-gated pipeline in one device pass (include/openglottal_hip_gated.h).

``GatedEngine(model, yolo)`` borrows a native ``UNet`` and a ``YoloV8Detector``: every source frame goes up once, the detector, the
temporal tracker (``k_track_boxes``: `openglottal/models/detector.py:61-96` on the device) and the U-Net run on it, and the areas
come back.  ``track_host`` is the tracker's host twin (the same inline function, no device); ``TemporalDetector.track`` wraps it.
"""

from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import OpenGlottalHipError, check, lib, ptr
from .utils import NET_SIZE


class TrackState(C.Structure):
    """``og_track_state``."""
    _fields_ = [("cx", C.c_float), ("cy", C.c_float), ("w", C.c_int32), ("h", C.c_int32), ("misses", C.c_int32), ("has_centre", C.c_int32)]

    def as_tuple(self):
        return (self.cx, self.cy, self.w, self.h, self.misses, self.has_centre)


class TrackParams(C.Structure):
    """``og_track_params``."""
    _fields_ = [("max_shift_px", C.c_float), ("padding", C.c_int32), ("max_hold_frames", C.c_int32)]


def params_of(max_shift_px=30, padding: int = 8, max_hold_frames: int = 3) -> TrackParams:
    return TrackParams(float(max_shift_px), int(padding), int(max_hold_frames))


def state_of_detector(det) -> TrackState:
    """The Python detector's ``_centre`` / ``_size`` / ``_misses`` as the six state words."""
    if det._centre is None:
        return TrackState(0.0, 0.0, 0, 0, 0, 0)
    return TrackState(float(det._centre[0]), float(det._centre[1]), int(det._size[0]), int(det._size[1]), int(det._misses), 1)


def state_to_detector(st: TrackState, det) -> None:
    if st.has_centre:
        det._centre = (np.float32(st.cx), np.float32(st.cy))
        det._size = (int(st.w), int(st.h))
        det._misses = int(st.misses)
    else:
        det._centre, det._size, det._misses = None, None, 0


def track_host(state: TrackState, params: TrackParams, best, W: int, H: int, resets=None) -> np.ndarray:
    """``og_track_host``: ``best [B,5]`` f32 through the tracker rule in order, from ``state`` (updated in place) → ``boxes [B,4]``
    int32 as ``utils.normalize_box`` leaves them.  ``resets [B]``: nonzero clears the state before that frame."""
    b = np.ascontiguousarray(best, dtype=np.float32).reshape(-1, 5)
    n = len(b)
    r = None if resets is None else np.ascontiguousarray(resets, dtype=np.uint8).reshape(n)
    boxes = np.empty((n, 4), np.int32)
    check(lib().og_track_host(C.addressof(state), C.addressof(params), ptr(b), ptr(r), n, int(W), int(H), ptr(boxes)), "og_track_host")
    return boxes


def plan(B: int, H: int, W: int, channels: int, stage_kib: int = 65536):
    """Dry run of the engine without a device: ``([(b0, nb), ...], engine_bytes)``."""
    out = C.create_string_buffer(1 << 20)
    nbytes = C.c_longlong()
    n = lib().og_gated_plan(B, H, W, channels, stage_kib, out, len(out), C.byref(nbytes))
    if n < 0:
        check(n, "og_gated_plan")
    mbs = [tuple(int(v) for v in line.split("|")) for line in out.value.decode().splitlines()]
    assert len(mbs) == n
    return mbs, nbytes.value


def gate_plan(B: int, H: int, W: int, channels: int, stage_kib: int = 65536, with_mask: bool = False):
    """Dry run of the ``skip_unboxed`` mode without a device: ``plan``'s micro-batches and the engine's device bytes in this mode."""
    out = C.create_string_buffer(1 << 20)
    nbytes = C.c_longlong()
    n = lib().og_gate_plan(B, H, W, channels, stage_kib, int(bool(with_mask)), out, len(out), C.byref(nbytes))
    if n < 0:
        check(n, "og_gate_plan")
    mbs = [tuple(int(v) for v in line.split("|")) for line in out.value.decode().splitlines()]
    assert len(mbs) == n
    return mbs, nbytes.value


def select_host(boxes) -> np.ndarray:
    """``og_gate_select_host``: the indices of the kept frames (``boxes[i][0] >= 0``: the tracker returned a box), ascending."""
    b = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
    keep = np.empty(len(b), np.int32)
    n = lib().og_gate_select_host(ptr(b), len(b), ptr(keep))
    if n < 0:
        check(n, "og_gate_select_host")
    return keep[:n].copy()


def _frame_args(frames):
    """``(array | None, keep-alive list | None, pointer array | None, B, H, W, channels)`` of an array or a list of u8 frames."""
    if isinstance(frames, (list, tuple)):
        keep = [f if (isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.flags.c_contiguous) else np.ascontiguousarray(f, dtype=np.uint8)
                for f in frames]
        if not keep:
            return None, keep, None, 0, 1, 1, 1
        shape = keep[0].shape
        if any(f.shape != shape for f in keep) or len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
            raise OpenGlottalHipError("GatedEngine: frames must share one [H,W] or [H,W,3] shape")
        ptrs = (C.c_void_p * len(keep))(*[f.ctypes.data for f in keep])
        return None, keep, ptrs, len(keep), shape[0], shape[1], 3 if len(shape) == 3 else 1
    f = np.ascontiguousarray(frames, dtype=np.uint8)
    if f.ndim == 4 and f.shape[-1] == 3:
        ch = 3
    elif f.ndim == 3:
        ch = 1
    else:
        raise OpenGlottalHipError(f"expected [B,H,W] or [B,H,W,3] frames, got {f.shape}")
    return f, None, None, f.shape[0], f.shape[1], f.shape[2], ch


class GatedEngine:
    """``og_gated``.  ``model``: a native ``UNet`` on its device; ``yolo``: a ``YoloV8Detector``.  Both are borrowed by the C handle;
    this object keeps them alive.  The tracker's state continues from ``run`` to ``run`` until ``reset``."""

    passes = 0   # device passes run by every engine of the process (tests: which path did `area_waveform` take?)

    def __init__(self, model, yolo, hold_yolo: bool = True) -> None:
        """``hold_yolo=False``: keep only a weak reference to ``yolo`` -- for an engine that ``yolo`` itself keeps (the cache of
        ``features.gated_engine_for``), which would otherwise keep its owner alive."""
        import weakref

        model._require()
        self.model = model
        self._yolo = yolo if hold_yolo else weakref.ref(yolo)
        self._imgsz = int(yolo.imgsz)
        self._uh, self._yh = model._h, yolo._h
        h = lib().og_gated_create(self._uh, self._yh)
        if not h:
            check(-1, "og_gated_create")
        self._h = h

    @property
    def yolo(self):
        import weakref

        return self._yolo() if isinstance(self._yolo, weakref.ref) else self._yolo

    def valid_for(self, model, yolo) -> bool:
        return (self._h is not None and model is self.model and yolo is self.yolo and model._h == self._uh and yolo._h == self._yh
                and int(yolo.imgsz) == self._imgsz)

    def set_option(self, name: str, value: int) -> None:
        check(lib().og_gated_set_option(self._h, name.encode(), int(value)), f"og_gated_set_option({name})")

    def reset(self) -> None:
        check(lib().og_gated_reset(self._h), "og_gated_reset")

    def set_params(self, max_shift_px=30, padding: int = 8, max_hold_frames: int = 3) -> None:
        p = params_of(max_shift_px, padding, max_hold_frames)
        check(lib().og_gated_set_params(self._h, C.addressof(p)), "og_gated_set_params")

    def get_state(self) -> TrackState:
        st = TrackState()
        check(lib().og_gated_get_state(self._h, C.addressof(st)), "og_gated_get_state")
        return st

    def set_state(self, st: TrackState) -> None:
        check(lib().og_gated_set_state(self._h, C.addressof(st)), "og_gated_set_state")

    def sync(self) -> None:
        check(lib().og_gated_sync(self._h), "og_gated_sync")

    def track_dev(self, best_dev, B: int, W: int, H: int, boxes_dev, resets_dev=None) -> None:
        """``og_track_boxes_dev`` on resident rows (torch CUDA tensors or raw ints); asynchronous."""
        check(lib().og_track_boxes_dev(self._h, ptr(best_dev), ptr(resets_dev), int(B), int(W), int(H), ptr(boxes_dev)), "og_track_boxes_dev")

    def run(self, frames, conf: float = 0.25, threshold: float = 0.5, resets=None, net=NET_SIZE, want_boxes: bool = True,
            want_best: bool = False, want_mask: bool = False, skip_unboxed: bool = False) -> dict:
        """The gated frame loop over ``frames`` (``[B,H,W]`` gray / ``[B,H,W,3]`` BGR u8 array, or a list of such frames of one
        shape) → ``{"area": int32 [B], "boxes": int32 [B,4] | None, "best": f32 [B,5] | None, "mask": u8 [B,H,W] | None}``
        (plus ``"kept": int`` with ``skip_unboxed``).  ``skip_unboxed``: the U-Net runs only on the frames the tracker gave a box; same ``area``,
        ``boxes`` and ``best``, the mask of a frame without a box is all zero, and ``"kept"`` counts the frames that were segmented."""
        arr, keep, ptrs, B, H, W, ch = _frame_args(frames)
        net_h, net_w = (int(net), int(net)) if np.isscalar(net) else (int(net[0]), int(net[1]))
        out = {"area": np.zeros(B, np.int32), "boxes": np.empty((B, 4), np.int32) if want_boxes else None,
               "best": np.empty((B, 5), np.float32) if want_best else None, "mask": np.empty((B, H, W), np.uint8) if want_mask else None}
        if skip_unboxed:
            out["kept"] = 0
        if B == 0:
            return out
        r = None if resets is None else np.ascontiguousarray(resets, dtype=np.uint8).reshape(B)
        l = lib()
        if skip_unboxed:
            fn, src = (l.og_gated_stream_kept_u8, ptr(arr)) if ptrs is None else (l.og_gated_stream_kept_frames_u8, ptrs)
        else:
            fn, src = (l.og_gated_stream_u8, ptr(arr)) if ptrs is None else (l.og_gated_stream_frames_u8, ptrs)
        kept = C.c_int32(0)
        extra = (C.addressof(kept),) if skip_unboxed else ()
        GatedEngine.passes += 1
        check(fn(self._h, src, B, H, W, ch, self._imgsz, net_h, net_w, float(conf), float(threshold), ptr(r), ptr(out["area"]),
                 ptr(out["boxes"]), ptr(out["best"]), ptr(out["mask"]), *extra), fn.__name__)
        if skip_unboxed:
            out["kept"] = int(kept.value)
        return out

    def segment_kept_dev(self, src, B: int, H: int, W: int, ch: int, boxes_dev, area_dev, mask_dev=None, threshold: float = 0.5,
                         net=NET_SIZE) -> int:
        """``og_gated_segment_kept_dev`` on resident frames (torch CUDA tensors or raw ints): the U-Net on the frames whose box has
        ``x1 >= 0`` only; ``area_dev`` / ``mask_dev`` come out in frame order, zero for the others.  Returns the number of kept
        frames; the work after the count is asynchronous on the U-Net's stream (``sync``)."""
        net_h, net_w = (int(net), int(net)) if np.isscalar(net) else (int(net[0]), int(net[1]))
        kept = C.c_int32(0)
        check(lib().og_gated_segment_kept_dev(self._h, ptr(src), int(B), int(H), int(W), int(ch), net_h, net_w, float(threshold),
                                              ptr(boxes_dev), ptr(mask_dev), ptr(area_dev), C.addressof(kept)), "og_gated_segment_kept_dev")
        return int(kept.value)

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().og_gated_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
