"""The crop-training cache of `scripts/train_unet_crop.py:84-162` (YOLO ROI) and `:225-297` (ground-truth ROI), built on the device:
``out_dir/<split>/images/%06d.png`` and ``masks/%06d.png`` (8-bit gray, ``crop_size`` squared, numbered over the kept samples in input
order) and ``meta.json`` with the keys `_cache_meta_valid` reads, so that the trainer finds a valid cache and skips its own pass.

Per sample: the ROI box (the detector's best row above ``conf``, or the tight box of ``label > 0``), padded by ``padding`` and clipped
to the frame; the image tile is ``k_crop_tiles`` of the frame (NEAREST letterbox of the crop, gray per tap: `letterbox_with_info`), the
mask tile ``k_crop_tiles<1>`` of the label with the same box (`letterbox_apply_geometry(..., INTER_NEAREST)`).  With ``decode="device"``
and ``encode="device"`` the files are decoded by ``PngDecoder``, the tiles made and PNG-coded on the device (``png.PngEncoder``,
include_enc/openglottal_hip_pnge.h) and only boxes and finished files cross the bus; ``"host"`` runs the same arithmetic through
``png.decode_host``, ``og_crop_tile_host`` and ``png.encode_host``: the twin the device is held to, byte for byte.

Skipped, as the reference skips them: a file without a detection; an empty label (``roi="gt"``); an empty box.  Also skipped: a box
whose letterboxed content rounds to zero pixels on a side (a sliver; `cv2.resize` raises on it in the reference).
Parity with a real cv2 is unpinned, as for every cv2 row of this project."""
from __future__ import annotations

import hashlib
import json
import os

import numpy as np

from . import png as P
from ._lib import OpenGlottalHipError, check, lib, ptr
from .features import _shape_runs


def source_hash(names) -> str:
    """`train_unet_crop.py:54-55`: the first 16 hex digits of the sha256 of the sorted file names joined by commas."""
    return hashlib.sha256(",".join(sorted(names)).encode()).hexdigest()[:16]


def yolo_box(best_row, H: int, W: int, padding: int):
    """`train_unet_crop.py:128-134`: the best row ``x1 y1 x2 y2 conf`` (conf < 0: no detection) -> the padded, clipped box or None."""
    x1, y1, x2, y2, conf = (float(v) for v in best_row)
    if conf < 0:
        return None
    return max(0, int(x1) - padding), max(0, int(y1) - padding), min(W, int(x2) + padding), min(H, int(y2) + padding)


def gt_box(tight, H: int, W: int, padding: int):
    """`train_unet_crop.py:261-271`: the tight box ``x_min y_min x_max+1 y_max+1`` of ``label > 0`` (all zero: an empty label) ->
    the padded, clipped box or None."""
    x0, y0, x1, y1 = (int(v) for v in tight)
    if x1 <= x0 or y1 <= y0:
        return None
    return max(0, x0 - padding), max(0, y0 - padding), min(W, x1 + padding), min(H, y1 + padding)


def usable(box, size: int) -> bool:
    """The box is not empty and both sides of its letterboxed content are at least one pixel (og_crop_usable's rule)."""
    if box is None or box[2] <= box[0] or box[3] <= box[1]:
        return False
    g = np.zeros(4, np.int32)
    check(lib().og_crop_geometry_host(box[3] - box[1], box[2] - box[0], int(size), ptr(g)), "og_crop_geometry_host")
    return bool(g[2] >= 1 and g[3] >= 1)


def crop_tile_host(frame: np.ndarray, box, size: int) -> np.ndarray:
    """``og_crop_tile_host``: ``[H,W,3]`` B G R or ``[H,W]`` gray -> the ``[size,size]`` gray tile of the box."""
    f = np.ascontiguousarray(frame, np.uint8)
    b = np.asarray(box, np.int32)
    tile = np.empty((size, size), np.uint8)
    check(lib().og_crop_tile_host(ptr(f), f.shape[0], f.shape[1], 3 if f.ndim == 3 else 1, ptr(b), int(size), ptr(tile)), "og_crop_tile_host")
    return tile


def label_bbox_host(label: np.ndarray):
    a = np.ascontiguousarray(label, np.uint8)
    b = np.zeros(4, np.int32)
    check(lib().og_pnge_label_bbox_host(ptr(a), a.shape[0], a.shape[1], ptr(b)), "og_pnge_label_bbox_host")
    return tuple(int(v) for v in b)


def _read(f) -> bytes:
    if isinstance(f, (bytes, bytearray, memoryview, np.ndarray)):
        return bytes(f)
    with open(os.fspath(f), "rb") as fh:
        return fh.read()


def _best_rows(detector, frames, conf: float, resident: bool) -> np.ndarray:
    """``best [n,5]`` of n frames of one shape: ``YoloV8Detector.detect_resized_dev`` on resident frames, ``detect_frames`` on host
    frames, or any callable ``(frames [n,H,W,3] u8, conf) -> [n,5]``."""
    d = getattr(detector, "model", detector)
    if resident and hasattr(d, "detect_resized_dev"):
        n, H, W = (int(v) for v in frames.shape[:3])
        return np.asarray(d.detect_resized_dev(frames, n, H, W, 3, conf), np.float32).reshape(-1, 5)
    f = frames.cpu().numpy() if resident else frames
    rows = d.detect_frames(f, conf) if hasattr(d, "detect_frames") else d(f, conf)
    return np.asarray(rows, np.float32).reshape(-1, 5)


def build(image_files, label_files, out_dir, split, roi: str = "yolo", detector=None, crop_size: int = 256, padding: int = 8,
          conf: float = 0.25, label_suffix: str = "", names=None, decode: str = "device", encode: str = "device", encoder=None,
          decoder=None) -> dict:
    """Writes the cache; returns ``{"n", "kept" (input indices), "boxes", "meta" (the dict written, or None when nothing was kept)}``.
    ``image_files`` / ``label_files``: paired paths or bytes of PNG files; ``names``: the file names the hash is taken over (default:
    the base names of ``image_files``, which must then be paths)."""
    image_files, label_files = list(image_files), list(label_files)
    if len(image_files) != len(label_files):
        raise OpenGlottalHipError(f"{len(image_files)} images but {len(label_files)} labels")
    if roi not in ("yolo", "gt"):
        raise OpenGlottalHipError(f"roi must be 'yolo' or 'gt', not {roi!r}")
    if roi == "yolo" and detector is None:
        raise OpenGlottalHipError("roi='yolo' needs a detector")
    if decode not in ("device", "host") or encode not in ("device", "host"):
        raise OpenGlottalHipError("decode and encode must be 'device' or 'host'")
    crop_size, padding = int(crop_size), int(padding)
    if crop_size < 1 or padding < 0:
        raise OpenGlottalHipError("crop_size must be positive and padding must not be negative")
    if names is None:
        names = [os.path.basename(os.fspath(f)) for f in image_files]
    img_dir, msk_dir = os.path.join(out_dir, split, "images"), os.path.join(out_dir, split, "masks")
    imgs_b, lbls_b = [_read(f) for f in image_files], [_read(f) for f in label_files]
    resident = decode == "device"
    if resident:
        dec = decoder if decoder is not None else P.PngDecoder()
        imgs = dec.decode_resident(imgs_b, 3) if imgs_b else []
        lbls = dec.decode_resident(lbls_b, 1) if lbls_b else []
    else:
        imgs = [P.decode_host(b, 3) for b in imgs_b]
        lbls = [P.decode_host(b, 1) for b in lbls_b]
    for i in range(len(imgs_b)):
        if tuple(imgs[i].shape[:2]) != tuple(lbls[i].shape[:2]):
            raise OpenGlottalHipError(f"pair {i}: the image is {tuple(imgs[i].shape[:2])}, its label {tuple(lbls[i].shape[:2])}")
    enc = None
    if resident or encode == "device":
        enc = encoder if encoder is not None else P.PngEncoder()
    kept, boxes, n = [], [], 0

    def write(tiles_files, mask_files):
        nonlocal n
        os.makedirs(img_dir, exist_ok=True)
        os.makedirs(msk_dir, exist_ok=True)
        for a, b in zip(tiles_files, mask_files):
            for d, data in ((img_dir, a), (msk_dir, b)):
                with open(os.path.join(d, f"{n:06d}.png"), "wb") as fh:
                    fh.write(data)
            n += 1

    for lo, hi in _shape_runs([_Shape(imgs[i]) for i in range(len(imgs_b))]):
        H, W = (int(v) for v in imgs[lo].shape[:2])
        if resident:
            import torch

            fr = imgs[lo:hi] if torch.is_tensor(imgs) else torch.stack(list(imgs[lo:hi]))
            lb = lbls[lo:hi] if torch.is_tensor(lbls) else torch.stack(list(lbls[lo:hi]))
            fr, lb = fr.contiguous(), lb.reshape(hi - lo, H, W).contiguous()
        else:
            fr, lb = np.stack(imgs[lo:hi]), np.stack([l[..., 0] for l in lbls[lo:hi]])
        if roi == "yolo":
            rows = _best_rows(detector, fr, conf, resident)
            if rows.shape[0] != hi - lo:
                raise OpenGlottalHipError(f"the detector gave {rows.shape[0]} rows for {hi - lo} frames")
            run_boxes = [yolo_box(r, H, W, padding) for r in rows]
        else:
            tight = enc.label_bbox_dev(lb, hi - lo, H, W).cpu().numpy() if resident else [label_bbox_host(l) for l in lb]
            run_boxes = [gt_box(t, H, W, padding) for t in tight]
        idx = [i for i, b in enumerate(run_boxes) if usable(b, crop_size)]
        if not idx:
            continue
        bx = np.array([run_boxes[i] for i in idx], np.int32)
        kept += [lo + i for i in idx]
        boxes += [tuple(int(v) for v in b) for b in bx]
        if resident:
            sel = torch.as_tensor(idx, device=fr.device)
            bx_dev = torch.from_numpy(bx).to(fr.device)
            tiles = enc.crop_tiles_dev(fr.index_select(0, sel).contiguous(), len(idx), H, W, 3, bx_dev, crop_size)
            masks = enc.crop_tiles_dev(lb.index_select(0, sel).contiguous(), len(idx), H, W, 1, bx_dev, crop_size)
        else:
            tiles = np.stack([crop_tile_host(fr[i], b, crop_size) for i, b in zip(idx, bx)])
            masks = np.stack([crop_tile_host(lb[i], b, crop_size) for i, b in zip(idx, bx)])
        if encode == "device":
            if resident:
                write(enc.files_resident(tiles, len(idx), crop_size, crop_size, 1), enc.files_resident(masks, len(idx), crop_size, crop_size, 1))
            else:
                write(enc.files(tiles), enc.files(masks))
        else:
            if resident:
                tiles, masks = tiles.cpu().numpy(), masks.cpu().numpy()
            write([P.encode_host(t) for t in tiles], [P.encode_host(m) for m in masks])
    meta = None
    if n:
        meta = {"n": n, "crop_size": crop_size, "label_suffix": label_suffix, "source_hash": source_hash(names), "roi_mode": roi}
        with open(os.path.join(out_dir, split, "meta.json"), "w") as fh:
            fh.write(json.dumps(meta, indent=2))
    return {"n": n, "kept": kept, "boxes": boxes, "meta": meta}


class _Shape:
    """What `features._shape_runs` looks at: a frame's shape and dtype, for host arrays and device tensors alike."""

    def __init__(self, a):
        self.shape, self.dtype = tuple(int(v) for v in a.shape), np.uint8


def cache_valid(out_dir, split, names, crop_size: int, label_suffix: str = "") -> bool:
    """`_cache_meta_valid` of `train_unet_crop.py:58-70`: what the trainer checks before it skips its own pass."""
    path = os.path.join(out_dir, split, "meta.json")
    if not os.path.exists(path):
        return False
    try:
        with open(path) as fh:
            meta = json.loads(fh.read())
        return meta.get("source_hash") == source_hash(names) and meta.get("crop_size") == crop_size and meta.get("label_suffix") == label_suffix
    except (json.JSONDecodeError, KeyError):
        return False


def list_pairs(images_dir: str, labels_dir: str, label_suffix: str = "", max_images: int = 0):
    """``(names, image paths, label paths)`` of `cli crop-cache`: the ``.png`` files of ``images_dir`` in name order (without the
    label files themselves when both directories are one), cut to ``max_images`` when that is not 0; the label of ``N.png`` is
    ``N<label_suffix>.png`` in ``labels_dir``.  ``names`` lists every image; the paths only the pairs whose label exists."""
    names = sorted(n for n in os.listdir(images_dir) if n.lower().endswith(".png") and not (label_suffix and n.endswith(label_suffix + ".png")))
    if max_images:
        names = names[:int(max_images)]
    pairs = [(os.path.join(images_dir, n), os.path.join(labels_dir, (n[:-4] + label_suffix + ".png") if label_suffix else n)) for n in names]
    pairs = [(a, b) for a, b in pairs if os.path.exists(b)]
    return names, [a for a, _ in pairs], [b for _, b in pairs]
