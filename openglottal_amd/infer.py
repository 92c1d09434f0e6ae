"""Annotated videos: the frame loops of `scripts/infer.py:129-265` (``_run_pipeline``) as batched device passes.  Each block of the
video is uploaded ONCE; the pipeline's existing ``*_dev`` entry leaves the mask and the area next to it, ``Overlay.annotate_dev``
draws, and only the annotated frames and 4 bytes of area per frame come back.  Device memory is that of
one block, not of the video.

Which mask is displayed follows the reference: the full-frame U-Net mask for ``unet`` (not cut to the box; none on a frame without a
box), the pasted crop mask for ``yolo-crop+unet``, every frame's mask and no rectangle for ``unet-only``, and for ``guided-vft`` no
mask on the seed frames, whose box is still drawn.  The text label is not drawn here (``overlay.label_host``).

``iter_pipeline_mjpeg`` is the same loop with ``mjpeg.Mjpeg`` behind the overlay: the annotated frames are
coded as JPEG files on the device and only those bytes come back, for ``mjpeg.AviWriter`` to put into ``<stem>_out.avi``.
"""
from __future__ import annotations

import csv
import os

import numpy as np

from ._lib import OpenGlottalHipError
from .features import YGVFT_INIT, YGVFT_PARAMS, _blocks_with_boxes, _kinematic_features, iter_frame_blocks
from .utils import NET_SIZE

PIPELINES = ("guided-vft", "unet", "unet-only", "yolo-crop+unet")
VFT_REFUSAL = ("--pipeline vft is not provided: its ROI comes from thresholding a Gaussian-blurred f32 motion map, which cannot be "
               "pinned without OpenCV (DESIGN.md section 15); use --pipeline guided-vft")
FEATURE_COLS = ["area_mean", "area_std", "area_range", "open_quotient", "f0", "periodicity", "cv"]


def _block_array(blk) -> np.ndarray:
    a = blk if isinstance(blk, np.ndarray) else np.stack([np.asarray(f) for f in blk])
    if a.dtype != np.uint8 or not (a.ndim == 3 or (a.ndim == 4 and a.shape[3] == 3)):
        raise OpenGlottalHipError(f"run_pipeline expects u8 frames [H,W] or [H,W,3] of one shape, got {a.dtype} {a.shape[1:]}")
    return np.ascontiguousarray(a)


def _iter_annotated_dev(frames_bgr, detector, pipeline, model, device=None, overlay_style="fill", threshold: float = 0.5,
                        crop_size: int = NET_SIZE, ygvft_init: int = YGVFT_INIT, overlay=None, skip_unboxed: bool = False):
    """The block loop that `iter_pipeline` and `iter_pipeline_mjpeg` share: ``(annotated [n,H,W,3] u8, area int32 [n])`` as CUDA
    tensors, block by block, in order; every handle has been waited for."""
    import torch

    from .overlay import Overlay, _style

    if pipeline == "vft":
        raise OpenGlottalHipError(VFT_REFUSAL)
    if pipeline not in PIPELINES:
        raise OpenGlottalHipError(f"pipeline must be one of {PIPELINES}, got {pipeline!r}")
    _style(overlay_style)
    kept_eng = None
    if skip_unboxed:
        from .features import _cached_gated_engine
        from .yolo import YoloV8Detector

        if pipeline != "unet":
            raise OpenGlottalHipError("skip_unboxed goes with pipeline 'unet' only: no other pipeline runs the U-Net on frames without a box")
        if type(getattr(detector, "model", None)) is not YoloV8Detector:
            raise OpenGlottalHipError("skip_unboxed needs the native detector backend (YoloV8Detector)")
    if pipeline != "guided-vft":
        if model is None:
            raise OpenGlottalHipError(f"--pipeline {pipeline} needs a U-Net")
        if device is not None and getattr(model, "_device", None) is None:
            model.to(device)
    if pipeline != "unet-only":
        if detector is None:
            raise OpenGlottalHipError(f"--pipeline {pipeline} needs a detector")
        detector.reset()
    dev = torch.device("cuda" if device is None else device)
    if dev.type == "cuda" and dev.index is None and getattr(model, "_device", None) is not None:
        dev = torch.device("cuda", model._device)
    ov = overlay if overlay is not None else Overlay()
    eng = None
    if pipeline == "guided-vft":
        from .classic import Classic

        if ygvft_init < 1:
            raise ValueError("ygvft_init must be at least 1")
        p = dict(YGVFT_PARAMS)
        eng = Classic(p["beta"], p["glottal_percentile"], p["max_glottal_components"], tiled="auto")
    seen, first_box, seeded = 0, None, False

    from .features import BLOCK
    from .mjpeg import CompressedVideo

    if isinstance(frames_bgr, CompressedVideo):
        # --decode device.  unet-only: the decoded block stays on the device and is `src` below.  With a
        # detector the video comes back to the host once, for the detector's existing frame loop.
        if pipeline == "unet-only":
            pairs = ((b, None) for b in frames_bgr.blocks_resident(BLOCK))
        else:
            pairs = _blocks_with_boxes(frames_bgr.frames_host(), detector, model)
    elif pipeline == "unet-only":
        pairs = ((b, None) for b in iter_frame_blocks(frames_bgr) if len(b))
    else:
        pairs = _blocks_with_boxes(frames_bgr, detector, model)
    with torch.cuda.device(dev):
        for blk, boxes in pairs:
            if torch.is_tensor(blk):                                      # decoded on the device: nothing to upload
                a, src = None, blk.to(dev)
                n, H, W = (int(v) for v in src.shape[:3])
                ch = 3
            else:
                a = _block_array(blk)
                n, H, W = a.shape[:3]
                ch = 3 if a.ndim == 4 else 1
                src = torch.from_numpy(a).to(dev)                         # the block's one upload
            bx = None if boxes is None else torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.int32)).to(dev)
            area = torch.zeros(n, dtype=torch.int32, device=dev)
            mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
            out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)                                   # (the handles below run on streams of their own)
            lo0 = 0                                                       # frames [0, lo0): no mask (guided-vft's seed frames)
            if skip_unboxed:
                kept_eng = kept_eng or _cached_gated_engine(detector.model, model)
                kept_eng.segment_kept_dev(src, n, H, W, ch, bx, area, mask_dev=mask, threshold=threshold, net=NET_SIZE)
                model.sync()                                              # (all of it ran on the U-Net's stream; the detector's is the worker's)
            elif pipeline in ("unet", "unet-only"):
                if (H, W) == (NET_SIZE, NET_SIZE):
                    gray = src
                    if ch == 3:
                        gray = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
                        model.bgr2gray_dev(src, n, H, W, gray)
                    model.segment_dev(gray, n, H, W, area, threshold, boxes_dev=bx, mask_dev=mask)
                else:
                    model.segment_resized_dev(src, n, H, W, ch, NET_SIZE, NET_SIZE, area, threshold, boxes_dev=bx, mask_dev=mask)
                model.sync()
            elif pipeline == "yolo-crop+unet":
                tiles = torch.empty((n, crop_size, crop_size), dtype=torch.uint8, device=dev)
                tmask = torch.empty_like(tiles)
                model.segment_crops_dev(src, n, H, W, ch, bx, crop_size, tiles, tmask, area_dev=area, mask_dev=mask, threshold=threshold)
                model.sync()
            else:
                if not seeded:
                    lo0 = min(n, ygvft_init - seen)
                    for i in range(lo0):
                        if first_box is None and boxes[i][0] >= 0:
                            first_box = tuple(int(v) for v in boxes[i])
                    seen += lo0
                    if seen >= ygvft_init:
                        eng.init([a[lo0 - 1]], first_box)
                        seeded = True
                if seeded and lo0 < n:
                    eng.guided_vft_dev(src[lo0:], n - lo0, H, W, ch, bx[lo0:], area[lo0:], mask_dev=mask[lo0:])
                    eng.sync()
            if lo0:
                ov.annotate_dev(src, lo0, H, W, ch, None, bx, out, overlay_style)
            if lo0 < n:
                ov.annotate_dev(src[lo0:], n - lo0, H, W, ch, mask[lo0:], None if bx is None else bx[lo0:], out[lo0:], overlay_style)
            ov.sync()
            yield out, area


def iter_pipeline(frames_bgr, detector, pipeline, model, device=None, overlay_style="fill", threshold: float = 0.5,
                  crop_size: int = NET_SIZE, ygvft_init: int = YGVFT_INIT, overlay=None, skip_unboxed: bool = False):
    """``(annotated [n,H,W,3] u8, area float64 [n])`` block by block, in order.  ``skip_unboxed`` (``pipeline="unet"`` with the native
    detector): the U-Net runs only on the frames with a box (``GatedEngine.segment_kept_dev``), as `infer.py:250-263`
    does; the annotated frames and the areas are the same bytes."""
    for out, area in _iter_annotated_dev(frames_bgr, detector, pipeline, model, device, overlay_style, threshold, crop_size, ygvft_init,
                                         overlay, skip_unboxed):
        yield out.cpu().numpy(), area.cpu().numpy().astype(np.float64)


def iter_pipeline_mjpeg(frames_bgr, detector, pipeline, model, device=None, overlay_style="fill", encoder=None, frames: bool = False,
                        **kw):
    """The same loop with the annotated frames coded as JPEG files on the device (``mjpeg.Mjpeg``): ``(blob u8, sizes
    int32 [n], area float64 [n])`` per block, the block's files back to back in ``blob``.  The frames go from ``Overlay.annotate_dev``
    into ``Mjpeg.encode_dev`` and never cross to the host uncompressed -- unless ``frames`` asks for them as a fourth item."""
    from .mjpeg import Mjpeg

    enc = encoder if encoder is not None else Mjpeg()
    for out, area in _iter_annotated_dev(frames_bgr, detector, pipeline, model, device, overlay_style, **kw):
        blob, sizes = enc.encode_resident(out)
        item = (blob, sizes, area.cpu().numpy().astype(np.float64))
        yield item + (out.cpu().numpy(),) if frames else item


def iter_pipeline_png(frames_bgr, detector, pipeline, model, device=None, overlay_style="fill", png_encoder=None, mjpeg_encoder=None,
                      frames: bool = False, **kw):
    """The same loop with the annotated frames coded as PNG files on the device (``png.PngEncoder``), and as JPEG files
    too when ``mjpeg_encoder`` is given: ``(files list[bytes], area float64 [n], jpeg (blob, sizes) or None, frames or None)`` per
    block.  The frames go from ``Overlay.annotate_dev`` into the coders and cross to the host uncompressed only if ``frames`` asks."""
    from .png import PngEncoder

    enc = png_encoder if png_encoder is not None else PngEncoder()
    for out, area in _iter_annotated_dev(frames_bgr, detector, pipeline, model, device, overlay_style, **kw):
        n, H, W = (int(v) for v in out.shape[:3])
        blob, sizes, total = enc.encode_resident(out, n, H, W, 3)
        jpeg = mjpeg_encoder.encode_resident(out) if mjpeg_encoder is not None else None
        enc.sync()
        sizes = sizes.cpu().numpy()
        data = blob[:int(total[0])].cpu().numpy()
        ends = np.cumsum(sizes.astype(np.int64))
        files = [data[int(e - k):int(e)].tobytes() for e, k in zip(ends, sizes)]
        yield files, area.cpu().numpy().astype(np.float64), jpeg, (out.cpu().numpy() if frames else None)


def run_pipeline(frames_bgr, detector, pipeline, model, device=None, overlay_style="fill", **kw):
    """``_run_pipeline``: ``(annotated [B,H,W,3] u8, area_wave float64 [B])`` for u8 frames of one shape (BGR, or gray, which is
    drawn on as B = G = R).  ``vft`` is refused with the sentence the CLI uses."""
    frames, waves = [], []
    for f, a in iter_pipeline(frames_bgr, detector, pipeline, model, device, overlay_style, **kw):
        frames.append(f)
        waves.append(a)
    if not frames:
        return np.zeros((0, 0, 0, 3), np.uint8), np.zeros(0, np.float64)
    return np.concatenate(frames), np.concatenate(waves)


# ── outputs of `cli infer` ────────────────────────────────────────────────────────────────────────────────────────────
class NpyWriter:
    """``<path>`` as ``np.save`` would write ``[B,H,W,3]`` u8, block by block through ``np.lib.format.open_memmap``."""

    def __init__(self, path: str, n_frames: int):
        self.path, self.n, self.at, self._mm = path, int(n_frames), 0, None

    def write(self, block: np.ndarray) -> None:
        if self._mm is None:
            self._mm = np.lib.format.open_memmap(self.path, mode="w+", dtype=np.uint8, shape=(self.n,) + tuple(block.shape[1:]))
        self._mm[self.at:self.at + len(block)] = block
        self.at += len(block)

    def close(self) -> None:
        if self._mm is not None:
            if self.at != self.n:
                raise OpenGlottalHipError(f"{self.path}: {self.at} of {self.n} frames written")
            self._mm.flush()
            self._mm = None


def features_row(stem: str, area_wave, capture_fps: float) -> dict:
    """One row of ``features.csv`` (`infer.py:436-445`): floats with four decimals, ``f0`` in Hz; every cell empty for a silent
    waveform.  The ``f0`` cell is left empty when ``f0`` is ``None`` (the reference raises there)."""
    feats = _kinematic_features([float(v) for v in area_wave])
    if feats is None:
        return {"source": stem, **{c: "" for c in FEATURE_COLS}}
    feats = dict(feats)
    feats["f0"] = None if feats["f0"] is None else feats["f0"] * capture_fps
    row = {"source": stem}
    for c in FEATURE_COLS:
        v = feats[c]
        row[c] = "" if v is None else (f"{v:.4f}" if isinstance(v, float) else v)
    return row


def write_features_csv(path: str, rows) -> None:
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["source"] + FEATURE_COLS)
        w.writeheader()
        for r in rows:
            w.writerow(r)


def write_pngs(directory: str, start: int, block: np.ndarray) -> None:
    from PIL import Image

    os.makedirs(directory, exist_ok=True)
    for i, f in enumerate(block):
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(os.path.join(directory, f"{start + i:06d}.png"))   # BGR -> RGB


def write_png_files(directory: str, start: int, files) -> None:
    """The files of ``iter_pipeline_png`` under the names ``write_pngs`` gives: ``%06d.png`` from ``start``."""
    os.makedirs(directory, exist_ok=True)
    for i, f in enumerate(files):
        with open(os.path.join(directory, f"{start + i:06d}.png"), "wb") as fh:
            fh.write(f)
