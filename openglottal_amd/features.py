"""`extract_features_unet`, `extract_features_yolo_guided_vft` and `_kinematic_features` (`openglottal/features.py`)."""

from __future__ import annotations

import os

import numpy as np

from ._lib import OpenGlottalHipError
from .utils import NET_SIZE, bgr_to_gray, normalize_box, unet_segment_frame

# Defaults of pipeline 2 (features.py:23-32).  alpha and gaussian_ksize drive the tracker's motion map, which reaches no output.
YGVFT_PARAMS = dict(alpha=0.98, beta=0.7, glottal_percentile=30, gaussian_ksize=13, max_glottal_components=2)
YGVFT_INIT = 2  # seed frames


def _kinematic_features(area_wave) -> dict | None:
    """Seven scalars of a glottal-area waveform (features.py:38-68).

    ``None`` for a silent (all-zero) waveform; ``f0`` is ``None`` when the
    spectral peak sits in the first non-DC bin; periodicity is the largest
    normalised autocorrelation over lags 1..49.
    """
    a = np.array(area_wave)
    if a.max() == 0:
        return None
    mu, sd = a.mean(), a.std()
    centred = a - mu
    spectrum = np.abs(np.fft.rfft(centred))
    k = int(np.argmax(spectrum[1:]) + 1)
    f0 = None if k == 1 else float(np.fft.rfftfreq(len(a))[k])
    full = np.correlate(centred, centred, mode="full")
    ac = full[len(full) // 2:]
    ac /= ac[0] + 1e-8
    return {
        "area_mean": mu,
        "area_std": sd,
        "area_range": a.max() - a.min(),
        "open_quotient": float(np.mean(a > mu * 0.1)),
        "f0": f0,
        "periodicity": float(ac[1:min(50, len(ac))].max()),
        "cv": sd / (mu + 1e-8),
        "_area": a,
    }


def load_frames_bgr(source) -> list[np.ndarray]:
    """Frames of a video as BGR u8 arrays (utils.py:43-54).

    ``source`` may be an in-memory array/list of frames, a ``.npy``/``.npz`` file
    (``[N,H,W,3]`` BGR or ``[N,H,W]`` gray), a directory of PNG/JPEG frames (Pillow), or a
    video file when OpenCV is importable (AVI/MJPG decode is host I/O and stays on cv2).  Without OpenCV an ``.avi``
    whose video stream is ``MJPG`` is read by ``mjpeg.read_avi_mjpeg``'s RIFF walk and Pillow; every other codec is still an error.
    """
    if isinstance(source, np.ndarray):
        return list(source)
    if isinstance(source, (list, tuple)):
        return list(source)
    p = str(source)
    if p.endswith(".npy"):
        return list(np.load(p))
    if p.endswith(".npz"):
        z = np.load(p)
        return list(z[z.files[0]])
    if not os.path.exists(p):
        return []
    if os.path.isdir(p):  # image-sequence directory (GIRAFE ships frames as PNGs): decode with Pillow, no OpenCV needed
        from PIL import Image

        frames = []
        for name in sorted(os.listdir(p)):
            if name.lower().endswith((".png", ".jpg", ".jpeg", ".bmp")):
                im = np.asarray(Image.open(os.path.join(p, name)))
                frames.append(np.ascontiguousarray(im[..., 2::-1]) if im.ndim == 3 else im)  # RGB(A) -> BGR, gray stays 2-D
        return frames
    try:
        import cv2  # noqa: F401
    except ImportError as e:
        from .mjpeg import avi_stream, decode_jpeg_bgr

        if p.lower().endswith(".avi"):   # Motion-JPEG, what `cli infer --avi device` writes: a RIFF walk and Pillow's decoder
            handler, chunks = avi_stream(p)
            if handler is not None and handler.upper() == b"MJPG":
                return [decode_jpeg_bgr(j) for j in chunks]
        raise OpenGlottalHipError(f"decoding {p} needs OpenCV; pass frames as .npy/.npz or an array instead") from e
    import cv2

    cap = cv2.VideoCapture(p)
    frames = []
    while True:
        ok, frm = cap.read()
        if not ok:
            break
        frames.append(frm)
    cap.release()
    return frames


BLOCK = 1024  # frames handed to the device engine per call (host side only: the engine itself streams micro-batches)
GATED_BLOCK = 128   # gated pipeline: the detector pass of block k + 1 runs (worker thread, own handle and stream) under the U-Net pass of
                    # block k; rounded up to a whole number of the model's micro-batches so that no block ends in a ragged launch


def gated_block(model) -> int:
    c = max(1, int(getattr(model, "chunk", 32)))
    return -(-GATED_BLOCK // c) * c


def iter_frame_blocks(source, block: int = BLOCK):
    """Blocks ``[n<=block,H,W(,3)]`` of a video without loading it whole where the container allows it: an ``.npy`` file is
    memory-mapped, an in-memory array is sliced (no copy), anything else goes through ``load_frames_bgr``."""
    if isinstance(source, str) and source.endswith(".npy") and os.path.exists(source):
        source = np.load(source, mmap_mode="r")
    if isinstance(source, np.ndarray) and source.ndim >= 3:
        for lo in range(0, len(source), block):
            yield source[lo:lo + block]
        return
    frames = source if isinstance(source, (list, tuple)) else load_frames_bgr(source)
    for lo in range(0, len(frames), block):
        yield frames[lo:lo + block]


def _detect_block(frames, detector) -> np.ndarray:
    """Boxes ``[n,4]`` int32 for one block; the temporal state machine carries over from the previous block."""
    n = len(frames)
    boxes = np.empty((n, 4), np.int32)
    batch = getattr(detector.model, "detect_frames", None)
    shapes = {f.shape for f in frames}
    if batch is not None and len(shapes) == 1:
        # native backend, frames of one size: the YOLO network is per-frame independent, so run it batched on the device
        # (letterboxed to the model's imgsz and scaled back exactly as the per-frame call does); only the O(1)/frame
        # temporal state machine (detector.py:61-96) is sequential
        best = batch(np.asarray(frames) if isinstance(frames, np.ndarray) else np.stack(frames), detector.conf)
        H, W = frames[0].shape[:2]
        for i in range(n):
            b = detector.update(best[i:i + 1, :4], best[i:i + 1, 4], W, H) if best[i, 4] >= 0 else detector.update(None, None, W, H)
            boxes[i] = normalize_box(b, W, H)
    else:
        for i, f in enumerate(frames):
            b = detector.detect(f)
            boxes[i] = normalize_box(b, f.shape[1], f.shape[0])
    return boxes


def _blocks_with_boxes(frames, detector, model=None):
    """``(block, boxes)`` pairs of the gated pipeline.  With the NATIVE detector backend (``detect_frames``: one batched device
    pass per block, the GIL released inside the C-ABI) the detector network and the O(1)-per-frame temporal state machine of block
    k + 1 run on ONE worker thread (so blocks are detected in order: the state machine is sequential, detector.py:61-96) while the
    caller segments block k.  Any other backend calls ``detector.detect`` per frame under the GIL -- a worker would overlap nothing --
    and keeps the plain sequential pass over BLOCK-sized blocks.  Nothing about the results changes either way: same boxes, in the
    same order, as a detect-everything-first pass.  (If the consumer abandons the generator, leaving the ``with`` block waits for
    the detection in flight -- at most one block.)"""
    from concurrent.futures import ThreadPoolExecutor

    if getattr(getattr(detector, "model", None), "detect_frames", None) is None:
        for blk in iter_frame_blocks(frames, BLOCK):
            if len(blk):
                yield blk, _detect_block(blk, detector)
        return
    it = (b for b in iter_frame_blocks(frames, gated_block(model)) if len(b))
    with ThreadPoolExecutor(1) as pool:
        nxt = next(it, None)
        fut = pool.submit(_detect_block, nxt, detector) if nxt is not None else None
        while nxt is not None:
            blk, boxes = nxt, fut.result()
            nxt = next(it, None)
            fut = pool.submit(_detect_block, nxt, detector) if nxt is not None else None
            yield blk, boxes


def _shape_runs(frames):
    """``(lo, hi)`` of each run of consecutive frames with one shape and dtype."""
    runs, lo = [], 0
    for i in range(1, len(frames) + 1):
        if i == len(frames) or frames[i].shape != frames[lo].shape or frames[i].dtype != frames[lo].dtype:
            runs.append((lo, i))
            lo = i
    return runs


def _u8_frames_of_one_shape(frames) -> bool:
    if isinstance(frames, np.ndarray):
        return frames.dtype == np.uint8 and len(frames) > 0 and (frames.ndim == 3 or (frames.ndim == 4 and frames.shape[3] == 3))
    f0 = frames[0] if len(frames) else None
    if not isinstance(f0, np.ndarray) or f0.dtype != np.uint8 or not (f0.ndim == 2 or (f0.ndim == 3 and f0.shape[2] == 3)):
        return False
    return all(isinstance(f, np.ndarray) and f.dtype == np.uint8 and f.shape == f0.shape for f in frames)


def gated_engine_for(frames, detector, model, policy: bool = True):
    """The device engine (``gated.GatedEngine``) when ``area_waveform(engine="auto")`` may take it for this call, else
    ``None``: a plain ``TemporalDetector`` (no method replaced on the instance, parameters plain numbers) on the native detector
    backend whose ``detect_frames`` is not overridden on the instance, a native ``UNet`` whose streamed entries are not overridden on
    the instance either, u8 gray or BGR frames of one shape, and -- unless ``policy`` is False, which is what ``engine="device"``
    passes -- a frame size at which the engine was measured ahead and a length at which both passes give the same bits.  The
    engine is kept on the detector backend and rebuilt when either network handle has changed."""
    from .detector import TemporalDetector
    from .unet import UNet
    from .yolo import YoloV8Detector

    if type(detector) is not TemporalDetector or type(detector.model) is not YoloV8Detector or type(model) is not UNet:
        return None
    if {"update", "detect", "reset", "track"} & set(vars(detector)) or "detect_frames" in vars(detector.model):
        return None
    if {"segment", "segment_stream", "segment_resized"} & set(vars(model)):
        return None   # an entry of the staged pass replaced on the model object: whoever did that wants to see its calls
    if not (isinstance(detector.max_shift, (int, float)) and isinstance(detector.padding, int) and isinstance(detector.max_hold_frames, int)):
        return None
    if not _u8_frames_of_one_shape(frames):
        return None
    if not policy:
        return _cached_gated_engine(detector.model, model)
    if tuple(frames[0].shape[:2]) == (NET_SIZE, NET_SIZE):
        # measured (profiles/gated_engine.json): at network size the staged pass already hides the detector under a
        # U-Net pass that runs on two lanes, and the engine's single-lane U-Net entry ends level with it or 2 % behind
        return None
    blk = gated_block(model)
    if blk % 256 == 1 or (len(frames) % blk) % 256 == 1:
        # the staged pass would hand a frame to the detector alone (its blocks go to the network 256 frames at a time), on the
        # one-frame latency kernels, whose sums run in another order; the engine runs every frame on the batched kernels.  Same
        # bits first: such a video stays staged.
        return None
    return _cached_gated_engine(detector.model, model)


def _cached_gated_engine(yolo, model):
    from .gated import GatedEngine

    cache = yolo.__dict__.setdefault("_gated_engines", {})     # on the backend: TemporalDetector objects come and go per video
    eng = cache.get(id(model))
    if eng is None or not eng.valid_for(model, yolo):
        model._require()
        if len(cache) >= 4:
            cache.clear()
        eng = cache[id(model)] = GatedEngine(model, yolo, hold_yolo=False)
    return eng


def _gated_device_pass(eng, frames, detector, threshold: float, skip_unboxed: bool = False) -> np.ndarray:
    """The whole video through the device engine in one call (it streams micro-batches itself); the Python detector is left in
    the state the staged pass would have left it in, so ``crop_size`` and a following ``detect()`` behave as before."""
    from . import gated

    detector.reset()
    eng.reset()
    eng.set_params(detector.max_shift, detector.padding, detector.max_hold_frames)
    src = frames if isinstance(frames, np.ndarray) and frames.flags.c_contiguous else list(frames)
    try:
        out = eng.run(src, conf=detector.conf, threshold=threshold, net=NET_SIZE, want_boxes=False, skip_unboxed=skip_unboxed)
    finally:
        gated.state_to_detector(eng.get_state(), detector)
    return out["area"].astype(np.float64)


def _segment_run(model, run, bx, threshold: float, skip_unboxed: bool) -> np.ndarray:
    """Areas of one run of equal-shape u8 frames through the model's streamed entry for its size.  ``skip_unboxed``: only the frames
    with a box (``bx[:, 0] >= 0``) are handed to the model, in order, and their areas scattered into zeros -- the same numbers, since
    a frame's area is a function of the frame and its box alone (analyze_gaw.py:86-95 segments no other frame either)."""
    at_net = run[0].shape[:2] == (NET_SIZE, NET_SIZE)
    if skip_unboxed and bx is not None:
        keep = np.flatnonzero(np.asarray(bx)[:, 0] >= 0)
        a = np.zeros(len(run), np.float64)
        if len(keep) == 0:
            return a
        if len(keep) < len(run):
            sub = run[keep] if isinstance(run, np.ndarray) else [run[i] for i in keep]
            a[keep] = _segment_run(model, sub, np.asarray(bx)[keep], threshold, False)
            return a
    if at_net:
        _, ar = model.segment_stream(run, threshold=threshold, boxes=bx)
    else:
        _, ar = model.segment_resized(run, net=NET_SIZE, threshold=threshold, boxes=bx, want_mask=False)
    return np.asarray(ar).astype(np.float64)


def area_waveform(frames, detector, model, device=None, threshold: float = 0.5, engine: str = "auto", skip_unboxed: bool = False) -> np.ndarray:
    """The frame loop of features.py:234-245 as batched device passes over blocks of the video.

    ``skip_unboxed`` (gated pass only): the U-Net runs only on the frames the detector gave a box, as
    `scripts/analyze_gaw.py:86-95` does; the waveform is the same.  The device engine compacts on the device
    (``GatedEngine.run(skip_unboxed=True)``), the staged pass on the host per run of one shape.

    ``engine``: ``"staged"`` is the host-stitched gated pass described below; ``"auto"`` (the default) takes the device engine of
    DESIGN §16 -- one upload per frame, detector, tracker and U-Net in one device pass, the same bits -- when
    ``gated_engine_for`` allows it, and the staged pass otherwise (mixed shapes, other dtypes, scripted or wrapped detectors, frames
    at network size, where the engine was measured level or behind); ``"device"`` insists on the engine and raises where it cannot run.

    U-Net-only (``detector is None``): area = #(mask>0) per frame.  Gated: the sequential TemporalDetector pass produces
    one box per frame first (the U-Net does not depend on it), then the fused kernel counts inside the boxes.  Frames at
    network size go to the streaming engine as they are — BGR included: `cv2.cvtColor(BGR2GRAY)` (features.py:235) runs on
    the device — so no per-frame host work is left and device memory does not grow with the video.  Frames of any other size
    (each run of one shape inside a mixed block) take the same engine with the two resizes of utils.py:234,239-240 on the device.
    """
    if engine not in ("auto", "staged", "device"):
        raise ValueError(f"engine must be 'auto', 'staged' or 'device', not {engine!r}")
    if device is not None and getattr(model, "_device", None) is None:
        model.to(device)
    if engine == "device" and detector is None:
        raise OpenGlottalHipError("engine='device' is the gated pass: it needs a detector")
    if engine != "staged" and detector is not None:
        if isinstance(frames, str) and frames.endswith(".npy") and os.path.exists(frames):
            frames = np.load(frames, mmap_mode="r")
        elif not isinstance(frames, (np.ndarray, list, tuple)):
            frames = load_frames_bgr(frames)   # (decoded once, whichever path takes them)
        eng = gated_engine_for(frames, detector, model, policy=engine == "auto")
        if eng is not None:
            return _gated_device_pass(eng, frames, detector, threshold, skip_unboxed)
        if engine == "device":
            raise OpenGlottalHipError("engine='device': this detector, model or video cannot take the device engine (gated_engine_for)")
    if detector is not None:
        detector.reset()
    out = []
    done = 0
    pairs = _blocks_with_boxes(frames, detector, model) if detector is not None else ((b, None) for b in iter_frame_blocks(frames))
    for blk, boxes in pairs:
        n = len(blk)
        if n == 0:
            continue
        shapes = {f.shape for f in blk}
        skip = skip_unboxed and boxes is not None
        if len(shapes) == 1 and next(iter(shapes))[:2] == (NET_SIZE, NET_SIZE) and not skip:
            # an array goes up in place; a list of frames (features.py:226's `frames_bgr`) is gathered by the engine itself,
            # frame by frame into its pinned ring -- no np.stack of the block
            _, area = model.segment_stream(blk if isinstance(blk, np.ndarray) else list(blk), threshold=threshold, boxes=boxes)
            out.append(area.astype(np.float64))
        else:   # other sizes / mixed sizes: each run of equal-shape u8 frames goes to the streamed resized entry
            a = np.zeros(n, np.float64)
            for lo, hi in _shape_runs(blk):
                run = blk[lo:hi]
                f0 = run[0]
                bx = None if boxes is None else boxes[lo:hi]
                if getattr(f0, "dtype", None) == np.uint8 and (f0.ndim == 2 or (f0.ndim == 3 and f0.shape[2] == 3)):
                    run = run if isinstance(run, np.ndarray) else list(run)
                    if skip:
                        ar = _segment_run(model, run, bx, threshold, True)
                    elif f0.shape[:2] == (NET_SIZE, NET_SIZE):
                        _, ar = model.segment_stream(run, threshold=threshold, boxes=bx)
                    else:
                        _, ar = model.segment_resized(run, net=NET_SIZE, threshold=threshold, boxes=bx, want_mask=False)
                    a[lo:hi] = ar
                    continue
                for i in range(lo, hi):   # not u8 gray / BGR: the per-frame loop of features.py:234-245
                    if skip and boxes[i][0] < 0:
                        continue
                    m = unet_segment_frame(bgr_to_gray(blk[i]), model, device, threshold)
                    if boxes is None:
                        a[i] = float(np.sum(m > 0))
                    elif boxes[i][0] >= 0:
                        x1, y1, x2, y2 = boxes[i]
                        a[i] = float(np.sum(m[y1:y2, x1:x2] > 0))
            out.append(a)
        done += n
    return np.concatenate(out) if out else np.zeros(0, np.float64)


def extract_features_unet(avi_path, detector, model, device=None, skip_unboxed: bool = False) -> dict | None:
    """Drop-in for `openglottal/features.py:202-247` (U-Net-only when ``detector is None``)."""
    wave = area_waveform(avi_path, detector, model, device, skip_unboxed=skip_unboxed)
    if len(wave) == 0:
        return None   # features.py:227-228
    return _kinematic_features([float(v) for v in wave])


def extract_gaw_features(frames, capture_fps, detector, model, device=None) -> dict | None:
    """`scripts/analyze_gaw.py:75-100` on top of ``area_waveform``: the detector is reset, the U-Net runs only on the frames with
    a box (``skip_unboxed=True``; a frame without one contributes area 0), the waveform goes through ``_kinematic_features`` and
    ``f0`` is scaled from cycles per frame to Hz.  ``None`` for a silent waveform; ``f0`` stays ``None`` where it is ``None``."""
    detector.reset()
    wave = area_waveform(frames, detector, model, device, skip_unboxed=True)
    feats = _kinematic_features([float(v) for v in wave])
    if feats is not None and feats["f0"] is not None:
        feats["f0"] *= capture_fps
    return feats


def crop_area_waveform(frames, detector, crop_model, device=None, threshold: float = 0.5, crop_size: int = NET_SIZE) -> np.ndarray:
    """The ``yolo-crop+unet`` frame loop of `scripts/infer.py:222-248` as batched device passes: per frame the detector's box
    is cropped out of the gray frame, letterboxed to ``crop_size``, segmented by the crop-trained U-Net and projected back;
    ``area = sum(mask_orig > 0)``, 0 for a frame without a box or with an empty crop.

    The blocks and their boxes come from ``_blocks_with_boxes``, unchanged: with the native detector backend the detector
    network and the temporal state machine of block k + 1 run on the worker thread under the crop pass of block k.  Each run of
    equal-shape u8 frames of a block (gray or BGR, any size) goes to ``UNet.segment_crops_stream``, which uploads and segments
    only the frames that have a usable box; device memory does not grow with the video.
    """
    if device is not None and getattr(crop_model, "_device", None) is None:
        crop_model.to(device)
    detector.reset()
    out = []
    for blk, boxes in _blocks_with_boxes(frames, detector, crop_model):
        a = np.zeros(len(blk), np.float64)
        for lo, hi in _shape_runs(blk):
            run = blk[lo:hi]
            f0 = run[0]
            if not (getattr(f0, "dtype", None) == np.uint8 and (f0.ndim == 2 or (f0.ndim == 3 and f0.shape[2] == 3))):
                run = [bgr_to_gray(f) for f in run]   # any other dtype / layout: the host conversion of infer.py:226
            _, ar = crop_model.segment_crops_stream(run if isinstance(run, np.ndarray) else list(run), boxes[lo:hi],
                                                    crop_size=crop_size, threshold=threshold)
            a[lo:hi] = ar
        out.append(a)
    return np.concatenate(out) if out else np.zeros(0, np.float64)


def extract_features_unet_crop(avi_path, detector, crop_model, device=None) -> dict | None:
    """`extract_features_unet` for the YOLO-Crop+UNet pipeline: the area waveform of `scripts/infer.py:222-248` into
    ``_kinematic_features``; ``None`` for an empty video or one without detections (an all-zero waveform)."""
    wave = crop_area_waveform(avi_path, detector, crop_model, device)
    if len(wave) == 0:
        return None
    return _kinematic_features([float(v) for v in wave])


def guided_vft_area_waveform(frames, detector, ygvft_init: int = YGVFT_INIT, params: dict | None = None) -> np.ndarray:
    """The frame loop of features.py:178-194 (YOLO-guided VFT) as batched device passes: the first ``ygvft_init`` frames seed the
    tracker (threshold from the last of them inside the first box seen among them) and contribute ``0.0``; every later frame is
    ``sum(process_frame(gray, box) > 0)``.

    The blocks and their boxes come from ``_blocks_with_boxes``, unchanged: with the native detector backend the detector network
    and the temporal state machine of block k + 1 run on the worker thread under the classical pass of block k.  Each run of
    equal-shape u8 frames (gray or BGR, any size) goes to ``Classic.guided_vft``; the threshold is carried on the device from
    call to call.  A video shorter than ``ygvft_init`` frames gives all zeros.
    """
    from .classic import Classic

    if ygvft_init < 1:
        raise ValueError("ygvft_init must be at least 1")
    p = dict(YGVFT_PARAMS, **(params or {}))
    eng = Classic(p["beta"], p["glottal_percentile"], p["max_glottal_components"], tiled="auto")
    detector.reset()
    out, seen, first_box, seeded = [], 0, None, False
    for blk, boxes in _blocks_with_boxes(frames, detector):
        n = len(blk)
        a = np.zeros(n, np.float64)
        lo0 = 0
        if not seeded:
            lo0 = min(n, ygvft_init - seen)
            for i in range(lo0):
                if first_box is None and boxes[i][0] >= 0:
                    first_box = tuple(int(v) for v in boxes[i])
            seen += lo0
            if seen >= ygvft_init:
                last = blk[lo0 - 1]
                eng.init([last if getattr(last, "dtype", None) == np.uint8 else bgr_to_gray(last)], first_box)
                seeded = True
        if seeded and lo0 < n:
            rest = blk[lo0:]
            for lo, hi in _shape_runs(rest):
                run = rest[lo:hi]
                f0 = run[0]
                if not (getattr(f0, "dtype", None) == np.uint8 and (f0.ndim == 2 or (f0.ndim == 3 and f0.shape[2] == 3))):
                    run = [bgr_to_gray(f) for f in run]   # any other dtype / layout: the host conversion of features.py:179
                _, ar = eng.guided_vft(run if isinstance(run, np.ndarray) else list(run), boxes[lo0 + lo:lo0 + hi], want_mask=False)
                a[lo0 + lo:lo0 + hi] = ar
        out.append(a)
    return np.concatenate(out) if out else np.zeros(0, np.float64)


def extract_features_yolo_guided_vft(avi_path, detector, ygvft_init: int = YGVFT_INIT) -> dict | None:
    """Drop-in for `openglottal/features.py:147-196`: ``None`` below ``ygvft_init + 2`` frames or for a silent waveform."""
    src = avi_path
    if isinstance(src, str) and src.endswith(".npy") and os.path.exists(src):
        src = np.load(src, mmap_mode="r")
    elif not isinstance(src, (np.ndarray, list, tuple)):
        src = load_frames_bgr(src)
    if len(src) < ygvft_init + 2:
        return None
    wave = guided_vft_area_waveform(src, detector, ygvft_init)
    return _kinematic_features([float(v) for v in wave])
