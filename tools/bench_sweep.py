#!/usr/bin/env python3
"""Measure the sweep (include/openglottal_hip_sweep.h) against what the library offered before it: a loop of `og_track_boxes_dev` +
`og_mask_stats_dev`, one pass per configuration.  Same build, same process, everything resident on the device; the timed window of
either ends in a synchronise.

    python tools/bench_sweep.py --frames 2000 --runs 5 --out profiles/sweep_bench.json
    rocprofv3 --kernel-trace --stats ... -- python tools/bench_sweep.py --only sweep --runs 3      (kernel times, a run of its own)

Grids: the paper's hold ablation (22 holds x 1 threshold), its confidence sweep (1 x 10 thresholds, every frame on its own) and
the full 22 x 10 grid.  Before anything is timed the two paths' counts are compared for equality.  The recorded ratio is the
SLOWEST sweep run over the FASTEST baseline run.  Inputs are seeded: noise masks and a scripted walk of detections; the cost of
either path does not depend on what the masks show.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_rows(n, H, W, seed=3):
    rs = np.random.RandomState(seed)
    best = np.zeros((n, 5), np.float32)
    cx, cy = W / 2.0, H / 2.0
    for i in range(n):
        if rs.rand() < 0.2:
            best[i, 4] = -1
            continue
        if rs.rand() < 0.05:
            cx, cy = rs.uniform(30, W - 30), rs.uniform(30, H - 30)
        cx = float(np.clip(cx + rs.uniform(-8, 8), 20, W - 20))
        cy = float(np.clip(cy + rs.uniform(-8, 8), 20, H - 20))
        w, h = rs.uniform(20, 90, 2)
        best[i] = (max(0, cx - w / 2), max(0, cy - h / 2), min(W, cx + w / 2), min(H, cy + h / 2), rs.uniform(0.0, 1.0))
    resets = np.zeros(n, np.uint8)
    resets[::250] = 1
    return best, resets


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--only", choices=["both", "sweep"], default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import openglottal_amd as og
    from openglottal_amd import gated, sweep, synth
    from openglottal_amd._lib import check, lib, ptr
    from openglottal_amd.yolo import YoloV8Detector

    n, H, W = a.frames, a.size, a.size
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(1)
    pred = torch.from_numpy(((rs.rand(n, H, W) < 0.2) * 255).astype(np.uint8)).to(dev)
    gt = torch.from_numpy(((rs.rand(n, H, W) < 0.2) * 255).astype(np.uint8)).to(dev)
    best, resets = make_rows(n, H, W)
    d_best = torch.from_numpy(best).to(dev)

    feats = (4, 8, 16, 32)     # the baseline's entries hang on a U-Net and a detector handle; neither network runs here
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5))
    m.to("cuda:0").eval()
    m._require()
    eng = gated.GatedEngine(m, YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0"))
    sw = sweep.Sweep()

    holds22 = list(range(21)) + [None]
    grids = {
        "hold 22x1": ([0.25], holds22, resets, False),
        "conf 1x10": (sweep.CONF_THRESHOLDS, [0], np.ones(n, np.uint8), True),
        "full 22x10": (sweep.CONF_THRESHOLDS, holds22, resets, False),
    }
    result = {"frames": n, "H": H, "W": W, "runs": a.runs, "device": torch.cuda.get_device_name(0), "grids": {}}
    for name, (thr, holds, rst, inclusive) in grids.items():
        Cn = len(thr) * len(holds)
        d_rst = torch.from_numpy(rst).to(dev)
        fc = torch.empty((n, 3), dtype=torch.int32, device=dev)
        cnt = torch.empty((Cn, n, 3), dtype=torch.int32, device=dev)
        # the baseline's pre-gated rows, one array per threshold (made outside the timed window)
        conf = best[:, 4].astype(np.float64)
        gated_rows = []
        for t in thr:
            rows = best.copy()
            rows[~((conf >= t) if inclusive else (conf > t)), 4] = -1
            gated_rows.append(torch.from_numpy(rows).to(dev))
        boxes = torch.empty((n, 4), dtype=torch.int32, device=dev)
        stats = torch.empty((Cn, n, 3), dtype=torch.int32, device=dev)
        stats_u = torch.empty((n, 3), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def run_sweep():
            sw.reset()
            sw.counts_dev(pred, gt, d_best, n, H, W, thr, holds, fc, cnt, resets_dev=d_rst, inclusive=inclusive)
            sw.sync()

        def run_baseline():
            check(lib().og_mask_stats_dev(m._h, ptr(pred), ptr(gt), n, H, W, None, ptr(stats_u)), "og_mask_stats_dev")
            for it in range(len(thr)):
                for ih, hold in enumerate(holds):
                    eng.set_params(30, 8, sweep.HOLD_FOREVER if hold is None else hold)
                    eng.reset()
                    eng.track_dev(gated_rows[it], n, W, H, boxes, d_rst)
                    eng.sync()                    # the tracker runs on the detector's stream, the counting on the U-Net's
                    check(lib().og_mask_stats_dev(m._h, ptr(pred), ptr(gt), n, H, W, ptr(boxes), ptr(stats[it * len(holds) + ih])),
                          "og_mask_stats_dev")
                    m.sync()                      # `boxes` is reused by the next configuration

        def timed(fn):
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3

        run_sweep()
        entry = {"configurations": Cn}
        if a.only == "both":
            run_baseline()
            s, c = stats.cpu().numpy(), cnt.cpu().numpy()
            assert np.array_equal(s[:, :, :2], c[:, :, :2]) and np.array_equal(stats_u.cpu().numpy(), fc.cpu().numpy()), name
            tb, ts = [], []
            for _ in range(a.runs):               # alternating, so that both see the same machine
                tb.append(timed(run_baseline))
                ts.append(timed(run_sweep))
            entry.update(baseline_ms=tb, sweep_ms=ts, slowest_sweep_over_fastest_baseline=max(ts) / min(tb),
                         median_baseline_over_median_sweep=float(np.median(tb) / np.median(ts)))
        else:
            entry["sweep_ms"] = [timed(run_sweep) for _ in range(a.runs)]
        # what either path must move at the least, from the shapes: the loop reads pred and gt once per configuration (and once for
        # the ungated row), the sweep reads them once and writes and reads its tables
        tab = 8 * (H + 1) * (W + 1)
        entry["bytes_baseline"] = (Cn + 1) * 2 * n * H * W
        entry["bytes_sweep"] = n * (2 * H * W + 3 * tab) + Cn * n * (4 * 8 + 12)
        result["grids"][name] = entry
        print(name, json.dumps(entry))
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
