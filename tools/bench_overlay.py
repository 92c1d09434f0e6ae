#!/usr/bin/env python
"""Annotated frames on the device against the host twin: same build, same process, legs alternating, five
runs each.

Per case (2 000 BGR frames at 256 x 256, 500 at 480 x 640) and style: ``Overlay.annotate`` (host in, host out, streamed) against
``overlay_host`` frame by frame, reported as the SLOWEST device run over the FASTEST host run; and ``annotate_dev`` alone on resident
buffers, timed by the handle's sync, from which the bytes per second of the pass follow under the stated model: C + 1 + 3 bytes per
pixel (source, mask, out) plus, for the outlined styles, the label traffic -- 4 bytes written by the tile pass and 4 read by the
overlay per pixel (seam, flatten and border passes touch a fraction of the array and are left out, so the figure is a floor).
Compared with the HBM rate a float4 copy reaches on this card.  Not a gate: `python tools/bench_overlay.py --out profiles/overlay_bench.json`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openglottal_amd import overlay as OV  # noqa: E402

HBM_COPY_TBS = 6.29      # measured float4 copy on an MI355X (8.0 TB/s spec)
RUNS = 5


def make_case(n, H, W, seed):
    rs = np.random.RandomState(seed)
    frames = rs.randint(0, 256, (n, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((n, H, W), np.uint8)
    boxes = np.zeros((n, 4), np.int32)
    for i in range(n):
        cy, cx = H / 2 + 6 * np.sin(i / 9.0), W / 2 + 4 * np.cos(i / 7.0)
        ry, rx = H / 5 * (0.6 + 0.4 * abs(np.sin(i / 5.0))), W / 14 * (0.6 + 0.4 * abs(np.sin(i / 5.0)))
        d = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
        m = d < 1.0
        m &= ~(d < 0.05)                                                   # a hole
        masks[i] = m * 255
        masks[i][rs.rand(H, W) < 0.002] = 255                              # specks
        boxes[i] = (int(cx - rx) - 8, int(cy - ry) - 8, int(cx + rx) + 8, int(cy + ry) + 8)
    boxes[::17] = -1                                                       # frames without a detection
    return frames, masks, boxes


def bytes_model(n, H, W, ch, style):
    return n * H * W * ((ch + 1 + 3) + (8 if style != "none" else 0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (a quick look)")
    a = ap.parse_args()
    import torch

    results = {"card": torch.cuda.get_device_name(0), "day": time.strftime("%Y-%m-%d"), "runs": RUNS, "hbm_copy_TBs": HBM_COPY_TBS,
               "model": "C + 1 + 3 bytes per pixel, + 8 label bytes per pixel for contour and fill", "cases": []}
    e = OV.Overlay()
    for n, H, W in ((int(2000 * a.scale), 256, 256), (int(500 * a.scale), 480, 640)):
        frames, masks, boxes = make_case(n, H, W, seed=H)
        d_f, d_m, d_b = torch.from_numpy(frames).cuda(), torch.from_numpy(masks).cuda(), torch.from_numpy(boxes).cuda()
        d_o = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        for style in ("none", "contour", "fill"):
            want = np.stack([OV.overlay_host(frames[i], masks[i], boxes[i], style, normalized=True) for i in range(min(n, 8))])
            assert np.array_equal(e.annotate(frames[:8], masks[:8], boxes[:8], style), want)      # (also the warm-up)
            e.annotate_dev(d_f, n, H, W, 3, d_m, d_b, d_o, style)
            e.sync()
            dev, host, res = [], [], []
            for _ in range(RUNS):                                          # legs alternating
                t = time.perf_counter()
                e.annotate(frames, masks, boxes, style)
                dev.append(time.perf_counter() - t)
                t = time.perf_counter()
                for i in range(n):
                    OV.overlay_host(frames[i], masks[i], boxes[i], style, normalized=True)
                host.append(time.perf_counter() - t)
                torch.cuda.synchronize()
                t = time.perf_counter()
                e.annotate_dev(d_f, n, H, W, 3, d_m, d_b, d_o, style)
                e.sync()
                res.append(time.perf_counter() - t)
            rate = bytes_model(n, H, W, 3, style) / max(res) / 1e12
            rec = {"frames": n, "H": H, "W": W, "style": style, "annotate_s": dev, "host_s": host, "annotate_dev_s": res,
                   "speedup_slowest_device_over_fastest_host": min(host) / max(dev),
                   "annotate_fps_slowest": n / max(dev), "host_fps_fastest": n / min(host),
                   "annotate_dev_TBs_slowest": rate, "annotate_dev_TBs_fastest": bytes_model(n, H, W, 3, style) / min(res) / 1e12,
                   "fraction_of_hbm_copy_slowest": rate / HBM_COPY_TBS}
            results["cases"].append(rec)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items() if not k.endswith("_s")}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
