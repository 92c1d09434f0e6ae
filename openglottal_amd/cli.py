"""``python -m openglottal_amd.cli run <video> --pipeline {guided-vft,unet,unet-only,yolo-crop+unet}`` and
``python -m openglottal_amd.cli infer --input DIR --mode {avi,images,npy} ...`` (annotated videos and ``features.csv``, below;
``--avi device`` writes them as Motion-JPEG ``<stem>_out.avi`` coded on the device, openglottal_amd/mjpeg.py), and
``python -m openglottal_amd.cli sweep --kind {hold,conf} --frames F.npy --gts G.npy ...`` (the paper's two ablations from one
inference pass, `openglottal_amd/sweep.py`).

Counterpart of the ``guided-vft`` branch and the two U-Net branches of `openglottal/cli.py:46-103` (`_cmd_run`), plus the
``yolo-crop+unet`` pipeline of `scripts/infer.py:222-248` (``--crop-weights``: the crop-trained U-Net checkpoint, `infer.py
--crop-weights`).  ``guided-vft`` (YOLO-guided VFT, training-free) needs ``--yolo-weights`` only; ``vft`` is refused with the reason
(its ROI depends on a Gaussian blur that cannot be pinned without OpenCV).  Same flags, same
`features.json` payload (every key of the feature dict incl. the ``_area`` waveform as a list, `cli.py:97`), same
messages; ``--annotate`` additionally records ``pipeline``/``video`` in the file.  ``<video>`` may be a ``.npy``/``.npz`` frame stack (or an AVI when OpenCV
is importable); weights are a torch ``state_dict`` file (U-Net, `weights_only=True`) and a flat
``.npz`` export (YOLO, see yolo.py).
"""
from __future__ import annotations

import argparse
import json
import os
import sys


def _precision_flags(r) -> None:
    r.add_argument("--precision", choices=["f32", "split", "f16"], default="f32", help="arithmetic of the U-Net, as for `run`")
    r.add_argument("--detector-precision", choices=["f32", "f16"], default="f32", help="arithmetic of the detector, as for `run`")


def add_infer_parser(sub):
    """`scripts/infer.py`'s flags, by name."""
    r = sub.add_parser("infer", help="annotated videos (mask fill and outline, detector box) and features.csv")
    r.add_argument("--input", required=True, help="a directory of videos (avi: *.avi, npy: *.npy frame stacks [B,H,W,3] u8), one .npy "
                                                  "file, or with --mode images a directory of images that are ONE sequence")
    r.add_argument("--mode", choices=["avi", "images", "npy"], default="avi")
    r.add_argument("--pipeline", choices=["vft", "guided-vft", "unet", "unet-only", "yolo-crop+unet"], default="unet")
    r.add_argument("--yolo-weights", default=None)
    r.add_argument("--unet-weights", default=None)
    r.add_argument("--crop-weights", default=None)
    r.add_argument("--output-dir", default="results")
    r.add_argument("--capture-fps", type=float, default=4000.0, help="capture frame rate in Hz: f0 is multiplied by it")
    r.add_argument("--max-hold-frames", type=int, default=3)
    r.add_argument("--overlay-style", choices=["fill", "contour", "none"], default="fill")
    r.add_argument("--device", default="cuda")
    r.add_argument("--frames", choices=["npy", "png"], default="npy", help="png: additionally a directory of PNGs per video (Pillow)")
    r.add_argument("--png", choices=["pillow", "device"], default="pillow",
                   help="--frames png: pillow (default): the annotated frames come to the host and Pillow writes them, as until now; "
                        "device: they are filtered, deflated and framed as PNG files on the device and only the files come back; the "
                        "decoded pixels are the same")
    r.add_argument("--skip-unboxed", action="store_true",
                   help="--pipeline unet: run the U-Net only on the frames the detector gave a box (the same frames and areas)")
    r.add_argument("--label", action="store_true",
                   help="draw `area=N` at (4, 14) on the host after the device pass, with Pillow's built-in font: the glyphs are NOT "
                        "OpenCV's Hershey glyphs, so the label's pixels differ from the reference's")
    r.add_argument("--avi", choices=["opencv", "device"], default="opencv",
                   help="opencv (default): <stem>_out.avi through OpenCV's MJPG writer when OpenCV is importable, as until now; device: "
                        "the annotated frames are coded as baseline JPEG on the device and written as a Motion-JPEG <stem>_out.avi at "
                        "25 fps, no OpenCV needed")
    r.add_argument("--jpeg-quality", type=int, default=75, help="--avi device: IJG quality 1..100")
    r.add_argument("--no-npy", action="store_true",
                   help="--avi device: do not write <stem>_out.npy; the annotated frames then never leave the device uncompressed")
    _decode_flag(r)
    _precision_flags(r)
    return r


def _decode_flag(r) -> None:
    r.add_argument("--decode", choices=["host", "device", "auto"], default="host",
                   help="host (default): videos are decoded on the host, as until now; device: an MJPG .avi (or a directory of .jpg "
                        "frames of one size) goes to the device compressed and is decoded there (baseline JPEG only), and so does a "
                        "directory of .png frames of one size (8-bit, not interlaced); auto: device, "
                        "and the host loop, with one line on stderr, when the decoder refuses the first frame")
    r.add_argument("--decode-split", choices=["off", "auto"], default="off",
                   help="with --decode device or auto.  off (default): a lane per restart interval, so a file without restart markers "
                        "(OpenCV's, FFmpeg's and Pillow's default) is one lane per frame; auto: such files are decoded by many lanes "
                        "that synchronise themselves (the same bytes), files with markers as before")


def _infer_jobs(a):
    """``(stem, frames)`` per video; frames: a memory-mapped array, or a list of BGR frames."""
    import numpy as np

    if a.mode == "npy":
        paths = [a.input] if os.path.isfile(a.input) else sorted(os.path.join(a.input, f) for f in os.listdir(a.input) if f.endswith(".npy"))
        for p in paths:
            yield os.path.splitext(os.path.basename(p))[0], np.load(p, mmap_mode="r")
    elif a.mode == "images":
        from PIL import Image

        exts = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")
        paths = sorted(os.path.join(a.input, f) for f in os.listdir(a.input) if f.lower().endswith(exts))
        if not paths:
            raise SystemExit(f"No images found in {a.input}")
        if a.decode != "host":
            from .mjpeg import open_compressed

            video = None
            if all(p.lower().endswith((".jpg", ".jpeg")) for p in paths):
                video = open_compressed(a.input, a.decode, a.decode_split)
            elif all(p.lower().endswith(".png") for p in paths):   # PNG frames of one size: inflate and unfilter on the device
                from .png import open_compressed as open_png

                video = open_png(a.input, a.decode)
            elif a.decode == "auto":
                print(f"--decode auto: {a.input} is decoded on the host: it holds images that are no .jpg files", file=sys.stderr)
            else:
                raise SystemExit(f"--decode device with --mode images needs a directory of .jpg frames only: {a.input}")
            if video is not None:
                yield os.path.basename(os.path.normpath(a.input)), video
                return
        frames = [np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB"))[..., ::-1]) for p in paths]
        yield os.path.basename(os.path.normpath(a.input)), frames
    else:
        from .features import load_frames_bgr

        paths = sorted(os.path.join(a.input, f) for f in os.listdir(a.input) if f.endswith(".avi"))
        if not paths:
            raise SystemExit(f"No .avi files found in {a.input}")
        for p in paths:
            video = None
            if a.decode != "host":
                from .mjpeg import open_compressed

                video = open_compressed(p, a.decode, a.decode_split)
            yield os.path.splitext(os.path.basename(p))[0], video if video is not None else load_frames_bgr(p)


def _cmd_infer(ap, a) -> int:
    from . import infer as I

    if a.pipeline == "vft":
        ap.error(I.VFT_REFUSAL)
    if a.skip_unboxed and a.pipeline != "unet":
        ap.error("--skip-unboxed goes with --pipeline unet only: no other pipeline runs the U-Net on frames without a box")
    if a.pipeline in ("unet", "unet-only") and not a.unet_weights:
        ap.error("--unet-weights is required for the unet and unet-only pipelines")
    if a.pipeline == "yolo-crop+unet" and not a.crop_weights:
        ap.error("--crop-weights is required for the yolo-crop+unet pipeline")
    if a.pipeline != "unet-only" and not a.yolo_weights:
        ap.error("--yolo-weights is required for the guided-vft, unet and yolo-crop+unet pipelines")
    device_avi = a.avi == "device"
    if device_avi and a.label:
        ap.error("--label draws on the host after the device pass, so it needs the annotated frames there; with --avi device they are "
                 "coded on the device before they leave it.  Drop one of the two")
    if device_avi and not 1 <= a.jpeg_quality <= 100:
        ap.error("--jpeg-quality must be 1..100")
    if a.no_npy and not device_avi:
        ap.error("--no-npy goes with --avi device only: without it the .npy is the only annotated output")
    if a.decode != "host" and a.mode == "npy":
        ap.error("--decode device and auto are for compressed input (--mode avi, or --mode images with .jpg frames); a .npy holds "
                 "decoded frames")
    device_png = a.png == "device"
    if device_png and a.frames != "png":
        ap.error("--png device goes with --frames png only: it says where those files are coded")
    if device_png and a.label:
        ap.error("--label draws on the host after the device pass, so it needs the annotated frames there; with --png device they are "
                 "coded on the device before they leave it.  Drop one of the two")
    if a.no_npy and a.frames == "png" and not device_png:
        ap.error("--frames png needs the annotated frames on the host, which --no-npy leaves on the device; --png device codes them there")
    import numpy as np

    from . import TemporalDetector, UNet
    from .overlay import label_host

    detector = model = None
    if a.pipeline != "unet-only":
        detector = TemporalDetector(a.yolo_weights, max_hold_frames=a.max_hold_frames, precision=a.detector_precision)
    if a.pipeline != "guided-vft":
        import torch

        model = UNet(1, 1, (32, 64, 128, 256)).to(a.device)
        model.load_state_dict(torch.load(a.crop_weights if a.pipeline == "yolo-crop+unet" else a.unet_weights, map_location="cpu",
                                         weights_only=True))
        model.eval()
        if a.precision != "f32":
            model.set_option("precision", {"split": 1, "f16": 2}[a.precision])
    cv2 = encoder = None
    if device_avi:
        from .mjpeg import AviWriter, Mjpeg

        encoder = Mjpeg(a.jpeg_quality)
    else:
        try:
            import cv2
        except ImportError:
            print("OpenCV is not importable: annotated videos are written as <stem>_out.npy ([B,H,W,3] u8, BGR), not .avi")
    png_encoder = None
    if device_png:
        from .png import PngEncoder

        png_encoder = PngEncoder()
    os.makedirs(a.output_dir, exist_ok=True)
    rows = []
    for stem, frames in _infer_jobs(a):
        print(f"\n[{stem}]  {len(frames)} frames")
        if not len(frames):
            print("  WARNING: no frames loaded, skipping.")
            continue
        out_npy = os.path.join(a.output_dir, f"{stem}_out.npy")
        out_avi = os.path.join(a.output_dir, f"{stem}_out.avi")
        w = None if a.no_npy else I.NpyWriter(out_npy, len(frames))
        avi = None
        wave, at = [], 0
        if device_png:
            # the block loop of iter_pipeline with the PNG coder (and, with --avi device, the JPEG coder) behind the overlay; the frames
            # come back only for the .npy and for OpenCV's writer
            for files, area, jpeg, blk in I.iter_pipeline_png(frames, detector, a.pipeline, model, a.device, a.overlay_style,
                                                              png_encoder=png_encoder, mjpeg_encoder=encoder, frames=not a.no_npy,
                                                              skip_unboxed=a.skip_unboxed):
                I.write_png_files(os.path.join(a.output_dir, f"{stem}_out"), at, files)
                if device_avi:
                    if avi is None:
                        H, W = np.asarray(frames[0]).shape[:2]
                        avi = AviWriter(out_avi, W, H, 25.0)
                    avi.write(*jpeg)
                elif cv2 is not None:
                    if avi is None:
                        avi = cv2.VideoWriter(out_avi, cv2.VideoWriter_fourcc(*"MJPG"), 25.0, (blk.shape[2], blk.shape[1]))
                    for f in blk:
                        avi.write(f)
                if w is not None:
                    w.write(blk)
                wave.append(area)
                at += len(files)
            if avi is not None:
                avi.close() if device_avi else avi.release()
                print(f"  Wrote {out_avi}")
        elif device_avi:
            # the block loop of iter_pipeline with the JPEG coder behind the overlay; the frames come back only for the .npy
            for item in I.iter_pipeline_mjpeg(frames, detector, a.pipeline, model, a.device, a.overlay_style, encoder=encoder,
                                              frames=not a.no_npy, skip_unboxed=a.skip_unboxed):
                blob, sizes, area = item[:3]
                if avi is None:
                    H, W = np.asarray(frames[0]).shape[:2]
                    avi = AviWriter(out_avi, W, H, 25.0)
                avi.write(blob, sizes)
                if w is not None:
                    w.write(item[3])
                    if a.frames == "png":
                        I.write_pngs(os.path.join(a.output_dir, f"{stem}_out"), at, item[3])
                wave.append(area)
                at += len(sizes)
            if avi is not None:
                avi.close()
                print(f"  Wrote {out_avi}")
        else:
            for blk, area in I.iter_pipeline(frames, detector, a.pipeline, model, a.device, a.overlay_style, skip_unboxed=a.skip_unboxed):
                if a.label:
                    blk = np.stack([label_host(f, v) for f, v in zip(blk, area)])
                w.write(blk)
                if a.frames == "png":
                    I.write_pngs(os.path.join(a.output_dir, f"{stem}_out"), at, blk)
                if cv2 is not None:
                    if avi is None:
                        avi = cv2.VideoWriter(out_avi, cv2.VideoWriter_fourcc(*"MJPG"), 25.0, (blk.shape[2], blk.shape[1]))
                    for f in blk:
                        avi.write(f)
                wave.append(area)
                at += len(blk)
            if avi is not None:
                avi.release()
        if w is not None:
            w.close()
            print(f"  Wrote {out_npy}")
        row = I.features_row(stem, np.concatenate(wave), a.capture_fps)
        if not row["area_mean"]:
            print("  WARNING: silent waveform — no glottis detected.")
        rows.append(row)
        for c in I.FEATURE_COLS:
            if row[c] != "":
                print(f"  {c}: {row[c]}")
    path = os.path.join(a.output_dir, "features.csv")
    I.write_features_csv(path, rows)
    print(f"\nFeatures saved to {path}")
    return 0


def add_sweep_parser(sub):
    """The paper's two ablations from ONE inference pass (openglottal_amd/sweep.py)."""
    r = sub.add_parser("sweep", help="hold-duration ablation (eval_girafe.py --max-hold-frames, every value at once) or confidence "
                                     "sweep (scripts/sweep_bagls_conf.py): the networks run once")
    r.add_argument("--kind", choices=["hold", "conf"], required=True)
    r.add_argument("--frames", required=True, help=".npy: [N,H,W,3] / [N,H,W] u8 frames (conf: also an object array of mixed sizes)")
    r.add_argument("--gts", required=True, help=".npy: ground-truth masks, one per frame")
    r.add_argument("--patients", default=None, help=".npy: one id per frame (hold: the tracker is reset at every change)")
    r.add_argument("--unet-weights", required=True)
    r.add_argument("--yolo-weights", required=True)
    r.add_argument("--crop-weights", default=None, help="conf: adds the yolo-crop+unet row")
    r.add_argument("--conf", type=float, default=0.25, help="hold: the detector's confidence threshold")
    r.add_argument("--canvas", type=int, default=256, help="conf: frames are letterboxed to this size")
    r.add_argument("--output-json", default=None)
    r.add_argument("--device", default="cuda")
    _precision_flags(r)
    return r


def _cmd_sweep(a) -> int:
    import numpy as np
    import torch

    from . import TemporalDetector, UNet, sweep

    def unet(path):
        m = UNet(1, 1, (32, 64, 128, 256)).to(a.device)
        m.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
        m.eval()
        if a.precision != "f32":
            m.set_option("precision", {"split": 1, "f16": 2}[a.precision])
        return m

    frames = list(np.load(a.frames, allow_pickle=True))
    gts = list(np.load(a.gts, allow_pickle=True))
    if len(frames) != len(gts):
        raise SystemExit(f"{a.frames} holds {len(frames)} frames, {a.gts} {len(gts)} masks")
    model = unet(a.unet_weights)
    detector = TemporalDetector(a.yolo_weights, conf=a.conf, precision=a.detector_precision)
    if a.kind == "conf":
        res = sweep.conf_sweep(frames, gts, model, detector, crop_model=unet(a.crop_weights) if a.crop_weights else None, canvas=a.canvas,
                               output_json=a.output_json)
        sweep.print_conf_table(res)
    else:
        patients = None if a.patients is None else list(np.load(a.patients, allow_pickle=True))
        res = sweep.hold_ablation(frames, gts, model, detector, patients=patients)
        sweep.print_hold_table(res)
        if a.output_json:
            os.makedirs(os.path.dirname(os.path.abspath(a.output_json)), exist_ok=True)
            with open(a.output_json, "w") as f:
                json.dump({"inf" if h is None else str(h): r["summary"] for h, r in res.items()}, f, indent=2)
    if a.output_json:
        print(f"Results saved → {a.output_json}")
    return 0


def add_crop_cache_parser(sub):
    """The pre-computation of `scripts/train_unet_crop.py` (openglottal_amd/cropcache.py)."""
    r = sub.add_parser("crop-cache", help="the crop trainer's cache (cache/<split>/images|masks/%%06d.png and meta.json), decoded, "
                                          "cropped and PNG-coded on the device")
    r.add_argument("--images", required=True, help="a directory of .png images")
    r.add_argument("--labels", required=True, help="the directory of their labels: N.png, or N<label-suffix>.png")
    r.add_argument("--out", required=True, help="the cache directory (the trainer's --cache-dir)")
    r.add_argument("--split", required=True)
    r.add_argument("--roi", choices=["yolo", "gt"], default="yolo", help="yolo: the detector's best box; gt: the label's tight box")
    r.add_argument("--yolo-weights", default=None)
    r.add_argument("--label-suffix", default="")
    r.add_argument("--crop-size", type=int, default=256)
    r.add_argument("--padding", type=int, default=8)
    r.add_argument("--conf", type=float, default=0.25)
    r.add_argument("--max-images", type=int, default=0)
    r.add_argument("--host", action="store_true", help="decode, crop and encode on the host: the twin the device is held to (same files)")
    return r


def _cmd_crop_cache(ap, a) -> int:
    if a.roi == "yolo" and not a.yolo_weights:
        ap.error("--yolo-weights is required for --roi yolo")
    if a.crop_size < 1:
        ap.error("--crop-size must be positive")
    if a.padding < 0:
        ap.error("--padding must not be negative")
    from . import cropcache

    names, images, labels = cropcache.list_pairs(a.images, a.labels, a.label_suffix, a.max_images)
    if not names:
        raise SystemExit(f"No .png images found in {a.images}")
    detector = None
    if a.roi == "yolo":
        from .yolo import load_detector_backend

        detector = load_detector_backend(a.yolo_weights)
    where = "host" if a.host else "device"
    res = cropcache.build(images, labels, a.out, a.split, roi=a.roi, detector=detector, crop_size=a.crop_size, padding=a.padding, conf=a.conf,
                          label_suffix=a.label_suffix, names=names, decode=where, encode=where)
    print(f"{res['n']} of {len(names)} samples kept -> {os.path.join(a.out, a.split)}")
    return 0


def add_augment_preview_parser(sub):
    """The trainer's augmented samples as files to look at (openglottal_amd/augment.py)."""
    r = sub.add_parser("augment-preview", help="K augmented image / mask pairs of a crop cache, augmented and PNG-coded on the device")
    r.add_argument("--cache", required=True, help="the cache directory `crop-cache --out` wrote")
    r.add_argument("--split", required=True)
    r.add_argument("--n", type=int, default=8, help="how many samples, from the first one on")
    r.add_argument("--seed", type=int, default=0)
    r.add_argument("--out", required=True, help="receives images/%%06d.png (round(I * 255)) and masks/%%06d.png (M * 255)")
    r.add_argument("--host", action="store_true", help="the host twins instead of the device (same files)")
    return r


def _cmd_augment_preview(ap, a) -> int:
    if a.n < 1:
        ap.error("--n must be positive")
    from . import augment

    k = augment.preview(a.cache, a.split, a.n, a.seed, a.out, host=a.host)
    print(f"{k} augmented pairs -> {a.out}")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="openglottal_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    add_infer_parser(sub)
    add_sweep_parser(sub)
    add_crop_cache_parser(sub)
    add_augment_preview_parser(sub)
    r = sub.add_parser("run")
    r.add_argument("video")
    r.add_argument("--pipeline", choices=["vft", "guided-vft", "unet", "unet-only", "yolo-crop+unet"], default="unet-only")
    r.add_argument("--unet-weights", default=None, help="U-Net checkpoint (required for --pipeline unet / unet-only)")
    r.add_argument("--yolo-weights", default=None)
    r.add_argument("--crop-weights", default=None, help="crop-trained U-Net checkpoint (required for --pipeline yolo-crop+unet)")
    r.add_argument("--device", default="cuda")
    r.add_argument("-o", "--output", default="output")
    r.add_argument("--annotate", action="store_true", help="also write the pipeline and video names into features.json")
    r.add_argument("--skip-unboxed", action="store_true",
                   help="--pipeline unet: run the U-Net only on the frames the detector gave a box (the same waveform)")
    r.add_argument("--precision", choices=["f32", "split", "f16"], default="f32",
                   help="f32: exact fp32 kernels (default, the parity reference); split: opt-in f16 hi/lo split precision "
                        "(2.5x faster, same reference fixtures and tolerance; fails loudly if an activation leaves the f16 range); "
                        "f16: opt-in half precision (f16 operands and stored activations, f32 accumulation; fastest, half the "
                        "memory; logits move by ~1e-2, so masks may differ from f32 where a logit is near zero)")
    r.add_argument("--detector-precision", choices=["f32", "f16"], default="f32",
                   help="arithmetic of the YOLOv8 detector (--pipeline unet), independent of --precision (which is the U-Net's): "
                        "f32 (default) or the opt-in f16 mode (f16 weights and activations, f32 accumulation, f32 logits; the "
                        "throughput mode of batched calls)")
    _decode_flag(r)
    a = ap.parse_args(argv)
    if a.cmd == "infer":
        return _cmd_infer(ap, a)
    if a.cmd == "sweep":
        return _cmd_sweep(a)
    if a.cmd == "crop-cache":
        return _cmd_crop_cache(ap, a)
    if a.cmd == "augment-preview":
        return _cmd_augment_preview(ap, a)
    crop =a.pipeline == "yolo-crop+unet"
    if a.skip_unboxed and a.pipeline != "unet":
        ap.error("--skip-unboxed goes with --pipeline unet only: no other pipeline runs the U-Net on frames without a box")
    if a.pipeline == "vft":
        ap.error("--pipeline vft is not provided: its ROI comes from thresholding a Gaussian-blurred f32 motion map, which cannot be "
                 "pinned without OpenCV (DESIGN.md section 15); use --pipeline guided-vft")
    if a.pipeline == "guided-vft":
        if not a.yolo_weights:
            ap.error("--yolo-weights is required for --pipeline guided-vft")
        from . import TemporalDetector, extract_features_yolo_guided_vft

        detector = TemporalDetector(a.yolo_weights, precision=a.detector_precision)
        if a.decode != "host":
            a.video = _decoded_on_device(a)
        return _save(a, extract_features_yolo_guided_vft(a.video, detector))
    if crop and not a.crop_weights:
        ap.error("--crop-weights is required for --pipeline yolo-crop+unet")
    if not crop and not a.unet_weights:
        r.error("the following arguments are required: --unet-weights")   # (argparse's own message: required unless yolo-crop+unet)

    import torch

    from . import TemporalDetector, UNet, extract_features_unet, extract_features_unet_crop

    if (a.pipeline == "unet" or crop) and not a.yolo_weights:
        ap.error(f"--yolo-weights is required for --pipeline {a.pipeline}")
    if a.decode != "host":                                                # (after every argument check: this touches the device)
        a.video = _decoded_on_device(a)
    model = UNet(1, 1, (32, 64, 128, 256)).to(a.device)   # (yolo-crop+unet: the crop model; --precision applies to it)
    model.load_state_dict(torch.load(a.crop_weights if crop else a.unet_weights, map_location="cpu", weights_only=True))
    model.eval()
    if a.precision != "f32":
        model.set_option("precision", {"split": 1, "f16": 2}[a.precision])
    detector = TemporalDetector(a.yolo_weights, precision=a.detector_precision) if (a.pipeline == "unet" or crop) else None
    return _save(a, extract_features_unet_crop(a.video, detector, model, a.device) if crop
                 else extract_features_unet(a.video, detector, model, a.device, skip_unboxed=a.skip_unboxed))


def _decoded_on_device(a):
    """`run --decode device`: the frames of an MJPG .avi (or a directory of .jpg frames) decoded on the device, block by block, and
    handed to the feature extractors as the in-memory array they already take.  `auto`: the path itself when the decoder refuses it."""
    from .mjpeg import open_compressed

    if str(a.video).endswith((".npy", ".npz")):
        raise SystemExit(f"--decode {a.decode} is for compressed input (an MJPG .avi or a directory of .jpg frames), not {a.video}")
    exts = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")
    names = [n for n in os.listdir(str(a.video)) if n.lower().endswith(exts)] if os.path.isdir(str(a.video)) else []
    if names and all(n.lower().endswith(".png") for n in names):   # a directory of .png frames only
        from .png import open_compressed as open_png

        video = open_png(str(a.video), a.decode)
    else:
        video = open_compressed(str(a.video), a.decode, a.decode_split)
    return a.video if video is None else video.frames_host()


def _save(a, feats) -> int:
    if feats is None:
        print("No glottis detected — check your weights or input video.")
        return 1
    os.makedirs(a.output, exist_ok=True)
    path = os.path.join(a.output, "features.json")
    save = {k: v.tolist() if hasattr(v, "tolist") else v for k, v in feats.items()}   # as cli.py:97: all keys, _area as a list
    if a.annotate:
        save.update(pipeline=a.pipeline, video=str(a.video))
    with open(path, "w") as f:
        json.dump(save, f, indent=2)
    print(f"Features saved to {path}")
    for k, v in feats.items():
        if not k.startswith("_"):
            print(f"  {k}: {v:.4f}" if isinstance(v, float) else f"  {k}: {v}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
