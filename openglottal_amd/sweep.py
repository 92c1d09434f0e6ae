"""Detector ablation sweeps from one inference pass (include/openglottal_hip_sweep.h).

The paper's hold-duration ablation (`eval_girafe.py --max-hold-frames h`, once per value) and its confidence sweep
(`scripts/sweep_bagls_conf.py`) are one computation: the networks run once, afterwards only the detector's decision parameters
change and with them the box that gates the U-Net mask.  ``Sweep`` is the handle: masks, ground truth and ``best`` rows in, the
confusion counts of every (threshold, hold) configuration out, the masks read once.  ``sweep_host`` is its host twin (the same
inline functions, no device).  ``hold_ablation`` and ``conf_sweep`` are the two figures.
"""

from __future__ import annotations

import ctypes as C
import json
import os

import numpy as np

from ._lib import check, lib, ptr
from .gated import TrackState
from .utils import NET_SIZE

HOLD_FOREVER = 2147483647
CONF_THRESHOLDS = [0.001, 0.005, 0.01, 0.02, 0.03, 0.05, 0.10, 0.15, 0.20, 0.25]   # sweep_bagls_conf.py:34
RAW_CONF = 0.001                                                                   # sweep_bagls_conf.py:36
PIPELINES = ["unet-only", "yolo+unet", "yolo-crop+unet"]


def _grid(conf_thres, max_hold):
    t = np.ascontiguousarray(np.atleast_1d(conf_thres), dtype=np.float64)
    h = np.ascontiguousarray([HOLD_FOREVER if v is None else int(v) for v in np.atleast_1d(np.asarray(max_hold, dtype=object))], dtype=np.int32)
    return t, h


def sweep_host(pred, gt, best, conf_thres, max_hold, resets=None, max_shift_px=30, padding: int = 8, inclusive: bool = False,
               states=None, want_boxes: bool = True) -> dict:
    """``og_sweep_host``: ``pred``, ``gt`` ``[N,H,W]`` u8, ``best [N,5]`` f32 → ``{"frame_counts": int32 [N,3], "counts": int32
    [C,N,3], "boxes": int32 [C,N,4] | None}``, C = ``len(conf_thres) * len(max_hold)``, configuration ``it * n_hold + ih``.
    ``max_hold``: ints, ``None`` = hold forever.  ``states``: a ctypes array of C ``TrackState`` to continue from (updated in place)."""
    p = np.ascontiguousarray(pred, dtype=np.uint8)
    g = np.ascontiguousarray(gt, dtype=np.uint8)
    N, H, W = p.shape
    assert g.shape == p.shape
    b = np.ascontiguousarray(best, dtype=np.float32).reshape(N, 5)
    r = None if resets is None else np.ascontiguousarray(resets, dtype=np.uint8).reshape(N)
    t, h = _grid(conf_thres, max_hold)
    Cn = len(t) * len(h)
    out = {"frame_counts": np.empty((N, 3), np.int32), "counts": np.empty((Cn, N, 3), np.int32),
           "boxes": np.empty((Cn, N, 4), np.int32) if want_boxes else None}
    check(lib().og_sweep_host(ptr(p), ptr(g), ptr(b), ptr(r), N, H, W, ptr(t), len(t), ptr(h), len(h), float(max_shift_px), int(padding),
                              int(bool(inclusive)), None if states is None else C.addressof(states), ptr(out["frame_counts"]),
                              ptr(out["counts"]), ptr(out["boxes"])), "og_sweep_host")
    return out


def plan(N: int, H: int, W: int, n_conf: int, n_hold: int, chunk: int = 0):
    """Dry run without a device: ``([(b0, nb), ...], workspace_bytes)``.  ``chunk`` 0: the default for the shape."""
    out = C.create_string_buffer(1 << 20)
    nbytes = C.c_longlong()
    n = lib().og_sweep_plan(int(N), int(H), int(W), int(n_conf), int(n_hold), int(chunk), out, len(out), C.byref(nbytes))
    if n < 0:
        check(n, "og_sweep_plan")
    mbs = [tuple(int(v) for v in line.split("|")) for line in out.value.decode().splitlines()]
    assert len(mbs) == n
    return mbs, nbytes.value


class Sweep:
    """``og_sweep``.  The tracker state of every configuration continues from call to call until ``reset`` (or another grid)."""

    def __init__(self) -> None:
        h = lib().og_sweep_create()
        if not h:
            check(-1, "og_sweep_create")
        self._h = h

    def set_chunk(self, chunk: int) -> None:
        check(lib().og_sweep_set_chunk(self._h, int(chunk)), "og_sweep_set_chunk")

    def reset(self) -> None:
        check(lib().og_sweep_reset(self._h), "og_sweep_reset")

    def sync(self) -> None:
        check(lib().og_sweep_sync(self._h), "og_sweep_sync")

    def get_state(self, c: int) -> TrackState:
        st = TrackState()
        check(lib().og_sweep_get_state(self._h, int(c), C.addressof(st)), "og_sweep_get_state")
        return st

    plan = staticmethod(plan)

    def counts_dev(self, pred_dev, gt_dev, best_dev, N: int, H: int, W: int, conf_thres, max_hold, frame_counts_dev, counts_dev,
                   boxes_dev=None, resets_dev=None, max_shift_px=30, padding: int = 8, inclusive: bool = False) -> None:
        """``og_sweep_counts_u8_dev`` on resident buffers (torch CUDA tensors or raw ints); the grid is given on the host.
        Asynchronous on the handle's stream: the caller's producers must be done (``sync`` of their handles) before the call."""
        t, h = _grid(conf_thres, max_hold)
        check(lib().og_sweep_counts_u8_dev(self._h, ptr(pred_dev), ptr(gt_dev), ptr(best_dev), ptr(resets_dev), int(N), int(H), int(W), ptr(t),
                                           len(t), ptr(h), len(h), float(max_shift_px), int(padding), int(bool(inclusive)),
                                           ptr(frame_counts_dev), ptr(counts_dev), ptr(boxes_dev)), "og_sweep_counts_u8_dev")

    def counts(self, pred, gt, best, conf_thres, max_hold, resets=None, max_shift_px=30, padding: int = 8, inclusive: bool = False,
               want_boxes: bool = True) -> dict:
        """``og_sweep_counts_u8``: host arrays in, the dict of ``sweep_host`` out."""
        p = np.ascontiguousarray(pred, dtype=np.uint8)
        g = np.ascontiguousarray(gt, dtype=np.uint8)
        N, H, W = p.shape
        assert g.shape == p.shape
        b = np.ascontiguousarray(best, dtype=np.float32).reshape(N, 5)
        r = None if resets is None else np.ascontiguousarray(resets, dtype=np.uint8).reshape(N)
        t, h = _grid(conf_thres, max_hold)
        Cn = len(t) * len(h)
        out = {"frame_counts": np.empty((N, 3), np.int32), "counts": np.empty((Cn, N, 3), np.int32),
               "boxes": np.empty((Cn, N, 4), np.int32) if want_boxes else None}
        check(lib().og_sweep_counts_u8(self._h, ptr(p), ptr(g), ptr(b), ptr(r), N, H, W, ptr(t), len(t), ptr(h), len(h), float(max_shift_px),
                                       int(padding), int(bool(inclusive)), ptr(out["frame_counts"]), ptr(out["counts"]), ptr(out["boxes"])),
              "og_sweep_counts_u8")
        return out

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().og_sweep_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _agg_rows(frame_counts, counts, with_detector_rows=("yolo+unet",)):
    """The reference's ``agg`` structure (eval_girafe.py:225-324) of ONE configuration from its integer counts."""
    from .evaluate import metrics_from_counts

    agg = {p: {"dice": [], "iou": [], "n_det": 0, "n_total": 0} for p in ("unet-only",) + tuple(with_detector_rows)}
    for (tp_u, np_u, ng), (tp, npred, det) in zip(frame_counts.tolist(), counts.tolist()):
        d, j = metrics_from_counts(tp_u, np_u, ng)
        agg["unet-only"]["dice"].append(d)
        agg["unet-only"]["iou"].append(j)
        agg["unet-only"]["n_total"] += 1
        d, j = metrics_from_counts(tp, npred, ng)
        a = agg["yolo+unet"]
        a["dice"].append(d)
        a["iou"].append(j)
        a["n_total"] += 1
        a["n_det"] += int(det)
    return agg


def _device_of(unet_model):
    import torch

    unet_model._require()
    return torch.device("cuda", unet_model._device or 0)


def _rows_from_backend(backend, frames, conf: float) -> np.ndarray:
    """A scripted ``backend(frame_bgr, conf) -> (xyxy, conf)`` frame by frame: its top candidate as a ``best`` row (-1: none)."""
    best = np.zeros((len(frames), 5), np.float32)
    best[:, 4] = -1
    for i, f in enumerate(frames):
        xyxy, cf = backend(f if f.ndim == 3 else np.repeat(f[..., None], 3, axis=-1), conf)
        if cf is not None and len(cf):
            k = int(np.argmax(cf))
            best[i] = (*np.asarray(xyxy, np.float32)[k], np.float32(cf[k]))
    return best


def _masks_on_device(grays, unet_model, dev, block: int = 512, direct: bool = False):
    """The full-frame U-Net masks of ``grays [N,H,W]`` as a resident tensor: ONE U-Net pass, the masks never leave the device at
    network size (``direct``: at any size, the network run on the frame as it is, as `evaluate_counts_device` does on its canvas);
    other sizes go through `unet_segment_frame` as `evaluate` does and are uploaded."""
    import torch

    from .utils import unet_segment_frame

    n, H, W = grays.shape
    if (H, W) != (NET_SIZE, NET_SIZE) and not direct:
        return torch.from_numpy(np.stack([unet_segment_frame(g, unet_model, None) for g in grays])).to(dev)
    masks = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    area = torch.empty(n, dtype=torch.int32, device=dev)
    for lo in range(0, n, block):
        hi = min(n, lo + block)
        d_gray = torch.from_numpy(np.ascontiguousarray(grays[lo:hi])).to(dev)
        unet_model.segment_dev(d_gray, hi - lo, H, W, area[lo:hi], mask_dev=masks[lo:hi])
        unet_model.sync()   # d_gray may be released now
    return masks


def hold_ablation(frames, gts, unet_model, detector, holds=(*range(21), None), patients=None) -> dict:
    """The paper's hold-duration ablation from ONE inference pass: ``{hold: {"agg": ..., "summary": ...}}`` where ``agg`` holds the
    ``unet-only`` and ``yolo+unet`` entries of ``evaluate(...)`` run with ``TemporalDetector(..., max_hold_frames=hold)`` (``None``:
    hold forever) and ``summary`` is ``summarize(agg)``.  ``patients``: per-frame ids; every configuration is reset at every change,
    as `evaluate` resets the detector."""
    import torch

    from .evaluate import summarize
    from .utils import bgr_to_gray

    frames = [np.asarray(f) for f in frames]
    n = len(frames)
    grays = np.stack([bgr_to_gray(f) for f in frames])
    gts = np.ascontiguousarray(np.stack([np.asarray(g) for g in gts]), dtype=np.uint8)
    H, W = grays.shape[1:]
    dev = _device_of(unet_model)
    patients = list(patients) if patients is not None else ["all"] * n
    resets = np.array([i == 0 or patients[i] != patients[i - 1] for i in range(n)], np.uint8)
    batch = getattr(detector.model, "detect_frames", None)       # the native backend: ONE batched pass, as `evaluate` takes it
    best = (np.ascontiguousarray(batch(np.stack(frames), detector.conf), dtype=np.float32) if batch is not None
            else _rows_from_backend(detector.model, frames, detector.conf))
    masks = _masks_on_device(grays, unet_model, dev)
    d_gt = torch.from_numpy(gts).to(dev)
    d_best = torch.from_numpy(best).to(dev)
    d_res = torch.from_numpy(resets).to(dev)
    holds = list(holds)
    fc = torch.empty((n, 3), dtype=torch.int32, device=dev)
    cnt = torch.empty((len(holds), n, 3), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    sw = Sweep()
    try:
        sw.counts_dev(masks, d_gt, d_best, n, H, W, [float(detector.conf)], holds, fc, cnt, resets_dev=d_res,
                      max_shift_px=detector.max_shift, padding=detector.padding, inclusive=False)
        sw.sync()
    finally:
        sw.close()
    fc_h, cnt_h = fc.cpu().numpy(), cnt.cpu().numpy()
    out = {}
    for k, hold in enumerate(holds):
        agg = _agg_rows(fc_h, cnt_h[k])
        out[hold] = {"agg": agg, "summary": summarize(agg)}
    return out


def conf_sweep(frames, gts, unet_model, detector, crop_model=None, confs=CONF_THRESHOLDS, canvas: int = NET_SIZE, inclusive: bool = True,
               output_json: str | None = None, want_agg: bool = False):
    """`scripts/sweep_bagls_conf.py` on the device: frames (mixed sizes) are letterboxed to ``canvas``, the detector runs ONCE at
    0.001 and the U-Nets once, every frame is on its own (all resets 1), then every threshold of ``confs`` gates the box
    (``inclusive``: the script's ``conf >= thr``; ``False``: the detector's own ``conf > thr``).  Returns the dict the script
    writes (``str(thr) -> pipeline -> dice_mean, iou_mean, dice_ge_05, det_recall, n_det, n_total``) and writes it to
    ``output_json`` when given; with ``want_agg`` also ``{thr: agg}`` with the per-frame lists.  The ``yolo-crop+unet`` row (only
    with ``crop_model``) does not depend on the threshold: its counts come once from the raw box and are gated on the host."""
    import torch

    from .evaluate import metrics_from_counts
    from .gated import params_of, track_host
    from .geometry import letterbox, letterbox_geometry

    n = len(frames)
    S = int(canvas)
    dev = _device_of(unet_model)
    img = np.stack([letterbox(np.asarray(f), S) for f in frames])
    gt = np.ascontiguousarray(np.stack([letterbox(np.asarray(g), S) for g in gts]), dtype=np.uint8)
    from .utils import bgr_to_gray

    grays = np.stack([bgr_to_gray(f) for f in img])
    yolo = detector.model if hasattr(detector, "model") else detector
    best = np.zeros((n, 5), np.float32)
    if hasattr(yolo, "detect_dev"):       # the native detector on the resident canvas, as evaluate_counts_device runs it
        for lo in range(0, n, 512):
            blk = img[lo:lo + 512]
            bgr = torch.from_numpy(np.ascontiguousarray(blk if blk.ndim == 4 else np.repeat(blk[..., None], 3, axis=-1))).to(dev)
            torch.cuda.synchronize(dev)
            best[lo:lo + 512] = yolo.detect_dev(bgr, len(blk), S, S, RAW_CONF)
    else:
        best = _rows_from_backend(yolo, img, RAW_CONF)
    masks = _masks_on_device(grays, unet_model, dev, direct=True)
    d_gt = torch.from_numpy(gt).to(dev)
    d_best = torch.from_numpy(best).to(dev)
    d_res = torch.ones(n, dtype=torch.uint8, device=dev)
    confs = [float(c) for c in confs]
    padding = int(getattr(detector, "padding", 8))
    max_shift = getattr(detector, "max_shift", 30)
    fc = torch.empty((n, 3), dtype=torch.int32, device=dev)
    cnt = torch.empty((len(confs), n, 3), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    sw = Sweep()
    try:
        sw.counts_dev(masks, d_gt, d_best, n, S, S, confs, [0], fc, cnt, resets_dev=d_res, max_shift_px=max_shift, padding=padding,
                      inclusive=inclusive)
        sw.sync()
    finally:
        sw.close()
    fc_h, cnt_h = fc.cpu().numpy(), cnt.cpu().numpy()
    crop = None
    if crop_model is not None:
        crop_model._require()
        raw = track_host(TrackState(), params_of(max_shift, padding, 0), best, S, S, np.ones(n, np.uint8))   # the raw box of every frame
        cb = np.full((n, 4), -1, np.int32)
        geo = np.zeros((n, 4), np.int32)
        for i, b in enumerate(raw):
            if b[0] < 0 or b[2] - b[0] <= 0 or b[3] - b[1] <= 0:
                continue
            cb[i] = b
            geo[i] = letterbox_geometry(int(b[3] - b[1]), int(b[2] - b[0]), NET_SIZE)
        crop = np.zeros((n, 3), np.int32)
        for lo in range(0, n, 512):
            hi = min(n, lo + 512)
            B = hi - lo
            d_gray = torch.from_numpy(np.ascontiguousarray(grays[lo:hi])).to(dev)
            d_cb, d_geo = torch.from_numpy(cb[lo:hi].copy()).to(dev), torch.from_numpy(geo[lo:hi].copy()).to(dev)
            tiles = torch.empty((B, NET_SIZE, NET_SIZE), dtype=torch.uint8, device=dev)
            tmask = torch.empty_like(tiles)
            mask_c = torch.empty((B, S, S), dtype=torch.uint8, device=dev)
            st_c = torch.empty((B, 3), dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            check(lib().og_unet_segment_crops_u8_dev(crop_model._h, ptr(d_gray), B, S, S, ptr(d_cb), ptr(d_geo), NET_SIZE, 0.5, ptr(tiles),
                                                     ptr(tmask), ptr(mask_c)), "og_unet_segment_crops_u8_dev")
            crop_model.sync()
            check(lib().og_mask_stats_dev(unet_model._h, ptr(mask_c), ptr(d_gt[lo:hi]), B, S, S, None, ptr(st_c)), "og_mask_stats_dev")
            unet_model.sync()
            crop[lo:hi] = st_c.cpu().numpy()
    results, aggs = {}, {}
    for k, thr in enumerate(confs):
        agg = _agg_rows(fc_h, cnt_h[k])
        if crop is not None:
            a = {"dice": [], "iou": [], "n_det": 0, "n_total": 0}
            for i in range(n):
                det = bool(cnt_h[k, i, 2])          # the gate's verdict on this frame: every frame is on its own, nothing is held
                d, j = metrics_from_counts(int(crop[i, 0]) if det else 0, int(crop[i, 1]) if det else 0, int(fc_h[i, 2]))
                a["dice"].append(d)
                a["iou"].append(j)
                a["n_total"] += 1
                a["n_det"] += int(det)
            agg["yolo-crop+unet"] = a
        aggs[thr] = agg
        results[str(thr)] = {
            pipe: {"dice_mean": float(np.mean(d["dice"])), "iou_mean": float(np.mean(d["iou"])),
                   "dice_ge_05": float(np.mean([x >= 0.5 for x in d["dice"]]) * 100),
                   "det_recall": d["n_det"] / d["n_total"] if d["n_total"] > 0 else None, "n_det": d["n_det"], "n_total": d["n_total"]}
            for pipe, d in agg.items() if d["dice"]}
    if output_json:
        os.makedirs(os.path.dirname(os.path.abspath(output_json)), exist_ok=True)
        with open(output_json, "w") as f:
            json.dump(results, f, indent=2)
    return (results, aggs) if want_agg else results


def print_conf_table(results) -> None:
    """The table of sweep_bagls_conf.py:243-269 from ``conf_sweep``'s result."""
    sep = "=" * 90
    print(sep)
    print(f"  {'Conf':>5}  {'Pipeline':<20}  {'Det.Recall':>10}  {'Dice':>8}  {'IoU':>8}  {'Dice>=0.5':>10}")
    print(sep)
    keys = list(results)
    n = 0
    for key in keys:
        for pipe in PIPELINES:
            d = results[key].get(pipe)
            if d is None:
                continue
            n = d["n_total"]
            dr = "1.000 *" if pipe == "unet-only" else f"{d['det_recall']:.3f}"
            print(f"  {float(key):>5.2f}  {pipe:<20}  {dr:>10}  {d['dice_mean']:>8.3f}  {d['iou_mean']:>8.3f}  {d['dice_ge_05']:>9.1f}%")
        if key != keys[-1]:
            print("  " + "─" * 86)
    print(sep)
    print("  * unet-only is threshold-independent (no YOLO gate).")
    print(f"  Evaluated on {n} frames.")


def print_hold_table(result) -> None:
    """One `print_table` row pair (eval_girafe.py:355-366) per hold duration."""
    sep = "─" * 76
    print(f"\n{sep}\n  {'Hold':>6}  {'Method':<18}  {'Det.Recall':>10}  {'Dice':>8}  {'IoU':>8}  {'Dice≥0.5':>10}\n{sep}")
    label = {"unet-only": "U-Net only", "yolo+unet": "YOLO+UNet"}
    for hold, r in result.items():
        for p, s in r["summary"].items():
            dr = "1.000 *" if p == "unet-only" else f"{s['det_recall']:.3f}"
            print(f"  {'inf' if hold is None else hold:>6}  {label[p]:<18}  {dr:>10}  {s['dice']:>8.3f}  {s['iou']:>8.3f}  {s['dice_ge_0.5_pct']:>9.1f}%")
    print(sep)
