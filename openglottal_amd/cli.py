"""``python -m openglottal_amd.cli run <video> --pipeline {guided-vft,unet,unet-only,yolo-crop+unet}``.

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


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="openglottal_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("video")
    r.add_argument("--pipeline", choices=["vft", "guided-vft", "unet", "unet-only", "yolo-crop+unet"], default="unet-only")
    r.add_argument("--unet-weights", default=None, help="U-Net checkpoint (required for --pipeline unet / unet-only)")
    r.add_argument("--yolo-weights", default=None)
    r.add_argument("--crop-weights", default=None, help="crop-trained U-Net checkpoint (required for --pipeline yolo-crop+unet)")
    r.add_argument("--device", default="cuda")
    r.add_argument("-o", "--output", default="output")
    r.add_argument("--annotate", action="store_true", help="also write the pipeline and video names into features.json")
    r.add_argument("--precision", choices=["f32", "split", "f16"], default="f32",
                   help="f32: exact fp32 kernels (default, the parity reference); split: opt-in f16 hi/lo split precision "
                        "(2.5x faster, same reference fixtures and tolerance; fails loudly if an activation leaves the f16 range); "
                        "f16: opt-in half precision (f16 operands and stored activations, f32 accumulation; fastest, half the "
                        "memory; logits move by ~1e-2, so masks may differ from f32 where a logit is near zero)")
    r.add_argument("--detector-precision", choices=["f32", "f16"], default="f32",
                   help="arithmetic of the YOLOv8 detector (--pipeline unet), independent of --precision (which is the U-Net's): "
                        "f32 (default) or the opt-in f16 mode (f16 weights and activations, f32 accumulation, f32 logits; the "
                        "throughput mode of batched calls)")
    a = ap.parse_args(argv)
    crop = a.pipeline == "yolo-crop+unet"
    if a.pipeline == "vft":
        ap.error("--pipeline vft is not provided: its ROI comes from thresholding a Gaussian-blurred f32 motion map, which cannot be "
                 "pinned without OpenCV (DESIGN.md section 15); use --pipeline guided-vft")
    if a.pipeline == "guided-vft":
        if not a.yolo_weights:
            ap.error("--yolo-weights is required for --pipeline guided-vft")
        from . import TemporalDetector, extract_features_yolo_guided_vft

        detector = TemporalDetector(a.yolo_weights, precision=a.detector_precision)
        return _save(a, extract_features_yolo_guided_vft(a.video, detector))
    if crop and not a.crop_weights:
        ap.error("--crop-weights is required for --pipeline yolo-crop+unet")
    if not crop and not a.unet_weights:
        r.error("the following arguments are required: --unet-weights")   # (argparse's own message: required unless yolo-crop+unet)

    import torch

    from . import TemporalDetector, UNet, extract_features_unet, extract_features_unet_crop

    if (a.pipeline == "unet" or crop) and not a.yolo_weights:
        ap.error(f"--yolo-weights is required for --pipeline {a.pipeline}")
    model = UNet(1, 1, (32, 64, 128, 256)).to(a.device)   # (yolo-crop+unet: the crop model; --precision applies to it)
    model.load_state_dict(torch.load(a.crop_weights if crop else a.unet_weights, map_location="cpu", weights_only=True))
    model.eval()
    if a.precision != "f32":
        model.set_option("precision", {"split": 1, "f16": 2}[a.precision])
    detector = TemporalDetector(a.yolo_weights, precision=a.detector_precision) if (a.pipeline == "unet" or crop) else None
    return _save(a, extract_features_unet_crop(a.video, detector, model, a.device) if crop
                 else extract_features_unet(a.video, detector, model, a.device))


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
