#!/usr/bin/env python3
"""The streamed YOLO-Crop+UNet pass (`UNet.segment_crops_stream`) against the staged path that existed before it, on the SAME
build in the SAME process, over a seeded synthetic BGR video (`synth.bench_frame_bgr`) with scripted boxes at a 70 % detection
rate (the reference's BAGLS figure is 68.8 %).

  (a) staged: host `bgr_to_gray` of the video, `evaluate.unet_on_crops` in blocks of 128 frames (whole block staged, full-frame
      masks back), `np.sum(mask[y1:y2, x1:x2] > 0)` per frame;
  (b) streamed: `segment_crops_stream(frames_bgr, boxes, want_mask=False)`.

Two shapes -- 2 000 frames of 256 x 256 and 512 frames of 480 x 640 --, --runs runs of each leg, alternating, after one warm-up
of each.  The areas of both legs must be equal.  Prints frames per second, the ratio by the project's convention (SLOWEST streamed
run over FASTEST staged run) and the device memory the streamed engine holds after its first pass (its high-water mark: ring and
arenas are kept), one JSON line per shape.  Exit status 1 if a ratio is below 1.

    python tools/bench_crop_stream.py [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FEATS = (32, 64, 128, 256)
CROP = 256
BLOCK = 128


def scripted_boxes(n, h, w, rate=0.7, seed=2024):
    import numpy as np

    rs = np.random.RandomState(seed)
    boxes = []
    for _ in range(n):
        hit, bw, bh, cx, cy = rs.rand() < rate, rs.randint(48, w // 2), rs.randint(48, h // 2), rs.rand(), rs.rand()
        x1, y1 = int(cx * (w - bw)), int(cy * (h - bh))
        boxes.append((x1, y1, x1 + bw, y1 + bh) if hit else None)
    return boxes


def staged(model, frames_bgr, boxes):
    import numpy as np

    from openglottal_amd import evaluate
    from openglottal_amd.utils import bgr_to_gray

    gray = bgr_to_gray(frames_bgr)
    area = np.zeros(len(boxes), np.int32)
    for lo in range(0, len(boxes), BLOCK):
        bx = boxes[lo:lo + BLOCK]
        masks = evaluate.unet_on_crops(gray[lo:lo + BLOCK], bx, model, crop_size=CROP)
        for i, b in enumerate(bx):
            if b is not None:
                x1, y1, x2, y2 = b
                area[lo + i] = np.sum(masks[i][y1:y2, x1:x2] > 0)
    return area


def streamed(model, frames_bgr, boxes):
    return model.segment_crops_stream(frames_bgr, boxes, crop_size=CROP, want_mask=False)[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    a = ap.parse_args()

    import numpy as np
    import torch

    import openglottal_amd as og
    from openglottal_amd import synth

    sd = synth.make_unet_state_dict(FEATS, seed=5, head_scale=3.0, head_bias=-2.5)
    rows, ok = [], True
    for n, h, w in ((2000, 256, 256), (512, 480, 640)):
        video = np.stack([synth.bench_frame_bgr(i, h, w) for i in range(n)])
        boxes = scripted_boxes(n, h, w)
        old = og.UNet(1, 1, FEATS).to("cuda:0").eval()
        new = og.UNet(1, 1, FEATS).to("cuda:0").eval()     # its own handle: the memory figure below is the streamed engine's alone
        old.load_state_dict(sd)
        new.load_state_dict(sd)
        want = staged(old, video, boxes)                     # warm-up of (a)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        got = streamed(new, video, boxes)                    # warm-up of (b)
        held = free0 - torch.cuda.mem_get_info(0)[0]
        assert np.array_equal(got, want), "the two paths disagree"
        t_old, t_new = [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            r_old = staged(old, video, boxes)
            t1 = time.perf_counter()
            r_new = streamed(new, video, boxes)
            t2 = time.perf_counter()
            assert np.array_equal(r_old, want) and np.array_equal(r_new, want), "the two paths disagree"
            t_old.append(t1 - t0)
            t_new.append(t2 - t1)
        fps_old, fps_new = [round(n / t, 1) for t in t_old], [round(n / t, 1) for t in t_new]
        row = {"frames": n, "shape": [h, w, 3], "detection_rate": round(sum(b is not None for b in boxes) / n, 3),
               "mean_area": round(float(want.mean()), 1), "staged_fps": fps_old, "streamed_fps": fps_new,
               "slowest_streamed_over_fastest_staged": round(min(fps_new) / max(fps_old), 3),
               "streamed_engine_device_mib": round(held / 2 ** 20, 1)}
        ok = ok and row["slowest_streamed_over_fastest_staged"] >= 1.0
        rows.append(row)
        print(json.dumps(row), flush=True)
        del old, new, video
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(r) for r in rows) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
