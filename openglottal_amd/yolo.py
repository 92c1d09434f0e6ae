"""Native YOLOv8 detector backend behind ``TemporalDetector`` (`openglottal/models/detector.py:31,58`).

``YoloV8Detector`` is what ``ultralytics.YOLO(path)`` is to the reference: constructed from a
weights file, called as ``model(frame_bgr, conf)``.  Differences a user must know:

* weights are a flat ``.npz`` / dict of ultralytics' own state_dict keys (export once, where
  ultralytics is installed: ``np.savez(out, **{k: v.cpu().numpy() for k, v in
  YOLO(pt).model.state_dict().items()})``) — an ultralytics ``.pt`` is a pickle of its class graph
  and cannot be read without the package (SURVEY §7 hard parts);
* the network arithmetic is restated from ultralytics' published sources: PARITY UNPINNED.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import OpenGlottalHipError, check, lib, ptr
from .unet import _device_index

STRIDE = 32
PRECISIONS = {"f32": 0, "f16": 2}   # og_yolo_set_option(h, "precision", v); the detector has no split precision


def letterbox_bgr(frame: np.ndarray, imgsz: int = 256, stride: int = STRIDE):
    """ultralytics LetterBox(auto=True): fit the long side to ``imgsz``, pad (114) to a stride multiple.
    Returns ``(img, gain, pad_x, pad_y)``.  Identity for frames whose sides are multiples of 32 and <= imgsz."""
    from .geometry import resize_linear

    h, w = frame.shape[:2]
    r = min(imgsz / h, imgsz / w)
    nw, nh = int(round(w * r)), int(round(h * r))
    dw, dh = (imgsz - nw) % stride, (imgsz - nh) % stride
    img = frame if (nw, nh) == (w, h) else resize_linear(frame, nw, nh)
    top, left = int(round(dh / 2 - 0.1)), int(round(dw / 2 - 0.1))
    bottom, right = int(round(dh / 2 + 0.1)), int(round(dw / 2 + 0.1))
    if top or bottom or left or right:
        img = np.pad(img, ((top, bottom), (left, right), (0, 0)), constant_values=114)
    return np.ascontiguousarray(img), r, left, top


class YoloV8Detector:
    """``precision="f16"`` (or ``set_option("precision", 2)``) selects the opt-in f16 mode: the weights of every MFMA conv rounded
    to f16 once, every stored activation rounded to f16 once, f32 accumulation in one fixed K order, f32 logits into the unchanged
    decode.  Measured on one MI355X (``profiles/yolo_f16_bench.json``): batched calls of 256 frames run
    at 117.6 k frames/s against 51.4 k in f32 (2.28 x).  A ONE-FRAME call (``__call__`` / ``submit``) gains nothing to speak of: f16 mode
    never splits K, where the f32 latency path does, and the call is bound by its ~58 launches either way -- median 557-560 us in
    f16 against 571-586 us in f32, about equal, f16 marginally faster.  Boxes and confidences move by the f16 rounding of the activations; per-frame and
    batched calls still return identical bits.  An activation beyond the f16 range fails the call with ``OG_ERANGE``."""

    def __init__(self, weights, nc: int = 1, imgsz: int = 256, device="cuda:0", precision: str = "f32") -> None:
        if precision not in PRECISIONS:
            raise OpenGlottalHipError(f"precision must be one of {sorted(PRECISIONS)}, not {precision!r}")
        if isinstance(weights, (str, os.PathLike)):
            p = str(weights)
            if p.endswith(".pt"):
                raise OpenGlottalHipError(
                    f"{p}: ultralytics .pt checkpoints are pickles of ultralytics classes; export the state_dict to .npz "
                    "where ultralytics is installed (see openglottal_amd/yolo.py)")
            z = np.load(p)
            weights = {k: z[k] for k in z.files}
        self.imgsz = imgsz
        self.nc = nc
        check(lib().og_init(_device_index(device)), "og_init")
        h = lib().og_yolo_create(nc)
        if not h:
            check(-1, "og_yolo_create")
        try:
            for k, v in weights.items():
                if hasattr(v, "detach"):
                    v = v.detach().cpu().numpy()
                v = np.asarray(v)
                if k.endswith("num_batches_tracked"):
                    v64 = np.ascontiguousarray(v, dtype=np.int64).reshape(-1)
                    check(lib().og_yolo_set_tensor(h, k.encode(), ptr(v64), (C.c_int64 * 1)(0), 0, _lib.OG_DTYPE_I64), k)
                    continue
                v = np.ascontiguousarray(v, dtype=np.float32)
                shp = (C.c_int64 * max(1, v.ndim))(*v.shape)
                check(lib().og_yolo_set_tensor(h, k.encode(), ptr(v), shp, v.ndim, _lib.OG_DTYPE_F32), f"set_tensor({k})")
            if precision != "f32":   # (f32 is the handle's default)
                check(lib().og_yolo_set_option(h, b"precision", PRECISIONS[precision]), "og_yolo_set_option(precision)")
            check(lib().og_yolo_finalize(h), "og_yolo_finalize")
        except Exception:
            lib().og_yolo_destroy(h)
            raise
        self._h = h
        self._geo = {}   # (H, W) -> is letterbox_bgr the identity for frames of this size?

    def set_option(self, name: str, value: int) -> None:
        """Options of the C-ABI (``og_yolo_set_option``): ``precision`` (0 f32 | 2 f16), ``latency_batch``, ``splitk_slots``, ``splitk_div``,
        ``source_stage_kib`` (KiB of source frames staged per upload of a resized call), ``source_mapped``."""
        check(lib().og_yolo_set_option(self._h, name.encode(), int(value)), f"og_yolo_set_option({name})")

    def detect_batch(self, frames_bgr: np.ndarray, conf: float = 0.25, want_pred: bool = False):
        """``[B,H,W,3]`` u8 BGR at network size (sides multiples of 32) → ``best [B,5]`` (+ ``pred [B,A,5]``)."""
        f = np.ascontiguousarray(frames_bgr, dtype=np.uint8)
        B, H, W, _ = f.shape
        best = np.empty((B, 5), np.float32)
        A = lib().og_yolo_num_anchors(self._h, H, W)
        if A < 0:
            check(A, "og_yolo_num_anchors")
        pred = np.empty((B, A, 5), np.float32) if want_pred else None
        check(lib().og_yolo_detect_u8(self._h, ptr(f), B, H, W, float(conf), ptr(best), ptr(pred)), "og_yolo_detect_u8")
        return (best, pred) if want_pred else best

    def detect_dev(self, bgr_dev, B: int, H: int, W: int, conf: float = 0.25) -> np.ndarray:
        """``[B,H,W,3]`` u8 BGR frames RESIDENT ON THE DEVICE at network size (sides multiples of 32) → ``best [B,5]`` on the
        host (20 bytes per frame come back)."""
        import torch

        best = torch.empty((B, 5), dtype=torch.float32, device=bgr_dev.device)
        check(lib().og_yolo_detect_u8_dev(self._h, ptr(bgr_dev), B, H, W, float(conf), ptr(best), None), "og_yolo_detect_u8_dev")
        check(lib().og_yolo_sync(self._h), "og_yolo_sync")
        return best.cpu().numpy()

    def letterbox_dev(self, frames) -> np.ndarray:
        """``[B,H,W,3]`` / ``[B,H,W]`` u8 frames of one size → the letterboxed batch ``[B,Hn,Wn,3]`` as ``k_letterbox_bgr`` writes it
        (``og_yolo_letterbox_u8_dev``): the parity tap against ``letterbox_bgr``."""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        B, H0, W0 = f.shape[:3]
        ch = 1 if f.ndim == 3 else f.shape[3]
        i = [C.c_int() for _ in range(6)]
        g = C.c_double()
        check(lib().og_yolo_letterbox_geometry(H0, W0, self.imgsz, *[C.byref(v) for v in i], C.byref(g)), "og_yolo_letterbox_geometry")
        out = np.empty((B, i[0].value, i[1].value, 3), np.uint8)
        src = lib().og_malloc(max(1, f.nbytes))
        dst = lib().og_malloc(max(1, out.nbytes))
        try:
            if not src or not dst:
                check(-1, "og_malloc")
            check(lib().og_memcpy_h2d(src, ptr(f), f.nbytes), "og_memcpy_h2d")
            check(lib().og_yolo_letterbox_u8_dev(self._h, src, B, H0, W0, ch, self.imgsz, dst), "og_yolo_letterbox_u8_dev")
            check(lib().og_yolo_sync(self._h), "og_yolo_sync")
            check(lib().og_memcpy_d2h(ptr(out), dst, out.nbytes), "og_memcpy_d2h")
        finally:
            for p_ in (src, dst):
                if p_:
                    lib().og_free(p_)
        return out

    def detect_resized_dev(self, src_dev, B: int, H: int, W: int, channels: int = 3, conf: float = 0.25) -> np.ndarray:
        """``[B,H,W,channels]`` u8 frames of any size RESIDENT ON THE DEVICE → ``best [B,5]`` in source pixels on the host."""
        import torch

        best = torch.empty((B, 5), dtype=torch.float32, device=src_dev.device)
        check(lib().og_yolo_detect_resized_u8_dev(self._h, ptr(src_dev), B, H, W, channels, self.imgsz, float(conf), ptr(best)),
              "og_yolo_detect_resized_u8_dev")
        check(lib().og_yolo_sync(self._h), "og_yolo_sync")
        return best.cpu().numpy()

    def last_launches(self) -> list:
        """``[(label, module)]`` of the last kernel chain, the labels ``YoloPlanner.plan`` gives (needs ``set_option("trace_launches", 1)``)."""
        buf = C.create_string_buffer(1 << 16)
        n = lib().og_yolo_last_launches(self._h, buf, len(buf))
        if n < 0:
            check(n, "og_yolo_last_launches")
        return [tuple(l.split("|")) for l in buf.value.decode().splitlines()]

    def cu_count(self) -> int:
        import torch

        return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)

    def launch_count(self, kernel: str) -> int:
        """Launches of ``k_letterbox_bgr`` / ``k_scale_boxes`` issued by this handle so far (for tests)."""
        n = lib().og_yolo_launch_count(self._h, kernel.encode())
        if n < 0:
            check(int(n), "og_yolo_launch_count")
        return int(n)

    def _native_geometry(self, shape, dtype):
        """``(channels, identity)`` when frames of this shape go through the device letterbox (u8, gray or BGR), else ``None``."""
        if dtype != np.uint8 or len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] != 3):
            return None
        key = (shape[0], shape[1])
        geo = self._geo.get(key)
        if geo is None:
            i = [C.c_int() for _ in range(6)]
            g = C.c_double()
            check(lib().og_yolo_letterbox_geometry(shape[0], shape[1], self.imgsz, *[C.byref(v) for v in i], C.byref(g)),
                  "og_yolo_letterbox_geometry")
            nh, nw, ch, cw, top, left = (v.value for v in i)
            geo = self._geo[key] = (nh, nw) == (ch, cw) == key and (g.value, left, top) == (1.0, 0, 0)
        return (1 if len(shape) == 2 else 3), geo

    def detect_frames(self, frames_bgr, conf: float = 0.25) -> np.ndarray:
        """Frames of ONE size ``[B,H,W,3]`` (or ``[B,H,W]`` gray) at their ORIGINAL resolution → ``best [B,5]`` in
        original-frame pixels (conf = -1: no detection): what the ultralytics predictor does per call of
        ``self.model(frame_bgr, conf=...)`` (detector.py:58) — letterbox to ``imgsz``, network, ``scale_boxes`` back,
        clip — for the whole batch in one device pass.  ``__call__`` is this with B = 1, so the batched callers
        (`features.area_waveform`, `evaluate.evaluate`, `dist.sharded_gated_area_waveform`) and the per-frame
        ``TemporalDetector.detect`` see the same boxes for every frame size, not only where the letterbox is the identity.

        u8 frames whose letterbox is NOT the identity go up at their own size (gray: one byte per pixel) and are letterboxed on
        the device (``og_yolo_detect_resized_u8``): the bits of ``detect_frames_host``, without its per-frame numpy
        resize.  Identity frames (sides multiples of 32, long side ``imgsz``) take ``detect_frames_host``'s path as before."""
        f = np.asarray(frames_bgr)
        nat = self._native_geometry(f.shape[1:], f.dtype) if f.ndim in (3, 4) and f.shape[0] else None
        if nat is None or nat[1]:
            return self.detect_frames_host(f, conf)
        f = np.ascontiguousarray(f)
        B, H0, W0 = f.shape[:3]
        best = np.empty((B, 5), np.float32)
        check(lib().og_yolo_detect_resized_u8(self._h, ptr(f), B, H0, W0, nat[0], self.imgsz, float(conf), ptr(best)),
              "og_yolo_detect_resized_u8")
        return best

    def detect_frames_host(self, frames_bgr, conf: float = 0.25) -> np.ndarray:
        """``detect_frames`` with the letterbox on the HOST (``letterbox_bgr`` per frame in numpy, ``np.stack``, the network at
        network size, the f32 scale-back): the specification the device path is held to bit for bit, and the path of frames
        whose letterbox is the identity."""
        f = np.asarray(frames_bgr)
        if f.ndim == 3:
            f = np.repeat(f[..., None], 3, axis=-1)
        B, H0, W0 = f.shape[:3]
        if B == 0:
            return np.zeros((0, 5), np.float32)
        first, gain, px, py = letterbox_bgr(f[0], self.imgsz)
        if first.shape == f[0].shape and (gain, px, py) == (1.0, 0, 0):
            imgs = f
        else:
            imgs = np.stack([first] + [letterbox_bgr(x, self.imgsz)[0] for x in f[1:]])
        best = self.detect_batch(imgs, conf).copy()
        hit = best[:, 4] >= 0
        if (gain, px, py) != (1.0, 0, 0):  # scale_boxes back to the original frame
            best[:, [0, 2]] = (best[:, [0, 2]] - np.float32(px)) / np.float32(gain)
            best[:, [1, 3]] = (best[:, [1, 3]] - np.float32(py)) / np.float32(gain)
        best[:, [0, 2]] = best[:, [0, 2]].clip(0, W0)
        best[:, [1, 3]] = best[:, [1, 3]].clip(0, H0)
        best[~hit, :4] = 0
        return best.astype(np.float32)

    def __call__(self, frame_bgr: np.ndarray, conf: float = 0.25):
        """Backend protocol of ``TemporalDetector``: → ``(xyxy [n,4] f32, conf [n] f32)``, n ∈ {0,1}: the
        top-confidence detection in ORIGINAL frame pixels (what detector.py:61-64 consumes)."""
        b = self.detect_frames(np.asarray(frame_bgr)[None], conf)[0]
        if b[4] < 0:
            return np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
        return b[None, :4].astype(np.float32), b[4:5].astype(np.float32)

    def submit(self, frame_bgr: np.ndarray, conf: float = 0.25) -> None:
        """First half of ``__call__`` (``og_yolo_detect_u8_begin``, or ``og_yolo_detect_resized_u8_begin`` for a u8 frame whose
        letterbox is not the identity: letterbox on the device): enqueue the detector's chain on its own stream, return.  ``result()`` delivers what ``__call__`` would have returned.  In the reference's frame loop
        (features.py:235-245) the box only gates the count of the U-Net's mask, so the U-Net call of the same frame fits in between."""
        f = np.asarray(frame_bgr)
        nat = self._native_geometry(f.shape, f.dtype)
        if nat is not None and not nat[1]:   # letterbox on the device; og_yolo_detect_u8_end delivers source-pixel boxes
            f = np.ascontiguousarray(f)
            check(lib().og_yolo_detect_resized_u8_begin(self._h, ptr(f), 1, f.shape[0], f.shape[1], nat[0], self.imgsz, float(conf)),
                  "og_yolo_detect_resized_u8_begin")
            self._pending = (f.shape[0], f.shape[1], 1.0, 0, 0)   # nothing left to scale in result()
            return
        if f.ndim == 2:
            f = np.repeat(f[..., None], 3, axis=-1)
        img, gain, px, py = letterbox_bgr(f, self.imgsz)
        img = np.ascontiguousarray(img, dtype=np.uint8)
        H, W = img.shape[:2]
        check(lib().og_yolo_detect_u8_begin(self._h, ptr(img), 1, H, W, float(conf)), "og_yolo_detect_u8_begin")
        self._pending = (f.shape[0], f.shape[1], gain, px, py)

    def result(self):
        """Second half of ``__call__``: ``(xyxy [n,4] f32, conf [n] f32)``, n ∈ {0,1}, in ORIGINAL frame pixels."""
        if getattr(self, "_pending", None) is None:
            raise OpenGlottalHipError("result() without submit()")
        H0, W0, gain, px, py = self._pending
        self._pending = None
        best = np.empty((1, 5), np.float32)
        check(lib().og_yolo_detect_u8_end(self._h, ptr(best)), "og_yolo_detect_u8_end")
        b = best[0]
        if b[4] < 0:
            return np.zeros((0, 4), np.float32), np.zeros(0, np.float32)
        if (gain, px, py) != (1.0, 0, 0):  # scale_boxes back to the original frame, as detect_frames
            b[[0, 2]] = (b[[0, 2]] - np.float32(px)) / np.float32(gain)
            b[[1, 3]] = (b[[1, 3]] - np.float32(py)) / np.float32(gain)
        b[[0, 2]] = b[[0, 2]].clip(0, W0)
        b[[1, 3]] = b[[1, 3]].clip(0, H0)
        return b[None, :4].astype(np.float32), b[4:5].astype(np.float32)

    def activation(self, name: str, B: int = 1, cap: int = 1 << 22) -> np.ndarray:
        """The first ``B`` frames of a named tensor of the last call, f32 ``[B,C,H,W]``; ``cap``: room for it, in floats."""
        dims = (C.c_int * 3)()
        buf = np.empty(cap, np.float32)
        check(lib().og_yolo_get_activation(self._h, name.encode(), B, ptr(buf), cap, dims), f"og_yolo_get_activation({name})")
        c, h, w = dims[0], dims[1], dims[2]
        return buf[: B * c * h * w].reshape(B, c, h, w).copy()

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().og_yolo_destroy(self._h)
                self._h = None
        except Exception:
            pass


class YoloPlanner:
    """Dry runs of the detector's launch decisions without a device (``og_yolo_plan``): an unfinalized handle that holds the
    tensors of ``weights`` (only their shapes are read)."""

    FIELDS = ("gx", "gy", "gz", "block", "lds", "ws", "cnt")

    def __init__(self, weights, nc: int = 1) -> None:
        h = lib().og_yolo_create(nc)
        if not h:
            check(-1, "og_yolo_create")
        self._h = h
        for k, v in weights.items():
            if k.endswith("num_batches_tracked"):
                continue
            v = np.ascontiguousarray(v, dtype=np.float32)
            shp = (C.c_int64 * max(1, v.ndim))(*v.shape)
            check(lib().og_yolo_set_tensor(h, k.encode(), ptr(v), shp, v.ndim, _lib.OG_DTYPE_F32), f"set_tensor({k})")
        self._buf = C.create_string_buffer(1 << 16)

    def plan_text(self, B: int, H: int, W: int, n_cu: int = 0, options: str = "", want_arena: bool = True) -> str:
        arena = C.c_longlong(0)
        n = lib().og_yolo_plan(self._h, B, H, W, n_cu, options.encode(), self._buf, len(self._buf), C.byref(arena) if want_arena else None)
        if n < 0:
            check(n, "og_yolo_plan")
        self.arena_bytes = arena.value if want_arena else None
        return self._buf.value.decode()

    def plan(self, B: int, H: int, W: int, n_cu: int = 0, options: str = "") -> list:
        """One dict per launch: kernel (the label), gx, gy, gz, block, lds, ws (split-K workspace bytes), cnt (arrival counters), module."""
        out = []
        for line in self.plan_text(B, H, W, n_cu, options).splitlines():
            f = line.split("|")
            out.append(dict(kernel=f[0], module=f[8], **{k: int(v) for k, v in zip(self.FIELDS, f[1:8])}))
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().og_yolo_destroy(self._h)
                self._h = None
        except Exception:
            pass


def nms(xyxy: np.ndarray, conf: np.ndarray, conf_thres: float = 0.25, iou_thres: float = 0.7, max_det: int = 300) -> np.ndarray:
    """Greedy single-class NMS over decoded candidates (host side; ultralytics defaults IoU 0.7, 300 dets)."""
    idx = np.flatnonzero(conf > conf_thres)
    idx = idx[np.argsort(-conf[idx], kind="stable")]
    area = (xyxy[:, 2] - xyxy[:, 0]) * (xyxy[:, 3] - xyxy[:, 1])
    keep = []
    while idx.size and len(keep) < max_det:
        i, rest = idx[0], idx[1:]
        keep.append(i)
        iw = np.clip(np.minimum(xyxy[i, 2], xyxy[rest, 2]) - np.maximum(xyxy[i, 0], xyxy[rest, 0]), 0, None)
        ih = np.clip(np.minimum(xyxy[i, 3], xyxy[rest, 3]) - np.maximum(xyxy[i, 1], xyxy[rest, 1]), 0, None)
        inter = iw * ih
        idx = rest[inter / (area[i] + area[rest] - inter + 1e-12) <= iou_thres]
    return np.array(keep, dtype=np.int64)


def load_detector_backend(path: str, precision: str = "f32"):
    return YoloV8Detector(path, precision=precision)
