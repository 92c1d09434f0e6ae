#!/usr/bin/env python3
"""The gated engine with the U-Net on the kept frames only (`og_gated_stream_kept_u8`) against the plain engine
(`og_gated_stream_u8`, section 16) on the SAME build, in the SAME process, on one card -- and `k_gate_gather` alone.

Recorded, not gated: the tool always exits 0 when every leg ran.  One child process per precision, under its own time limit, one
after the other.  Inside a child, per frame size and per kept fraction: a warm-up of the plain engine, then the FIRST kept pass
(buffers allocated, the U-Net's graphs for the new batch sizes instantiated: reported separately), then the two legs alternate
(plain, kept, plain, kept, ...) --reps times each; a row reports every run and the SLOWEST kept run over the FASTEST plain run.

The kept fraction of a row is set by the confidence threshold: a quantile of the detector's own raw confidences on the frames, with
the tracker told to accept every detection and to hold none (max_shift_px 1e9, max_hold_frames 0), so that a frame is kept iff its
confidence exceeds the threshold; the achieved fraction is reported.  Input: seeded noise frames (100 distinct frames, tiled) in
pageable memory.

    python tools/bench_gate.py [--reps 5] [--out profiles/gate_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((2000, 256, 256), (512, 480, 640))
FRACTIONS = (0.3, 0.7, 1.0)
GATHER_SHAPES = ((512, 480, 640, 3), (512, 479, 639, 3))     # rows of 921600 bytes (a multiple of 16) and of 918243 (odd)


def gather_leg(e, reps):
    import numpy as np
    import torch

    from openglottal_amd._lib import check, lib

    rows = []
    for B, h, w, c in GATHER_SHAPES:
        rb = h * w * c
        keep = np.sort(np.random.RandomState(B).choice(B, int(0.7 * B), replace=False)).astype(np.int32)
        n = len(keep)
        src = torch.randint(0, 256, (B * rb,), dtype=torch.uint8, device="cuda:0")
        dst = torch.empty((n * rb,), dtype=torch.uint8, device="cuda:0")
        d_keep = torch.from_numpy(keep).to("cuda:0")
        torch.cuda.synchronize()

        def once(iters):
            t = time.perf_counter()
            for _ in range(iters):
                check(lib().og_gate_gather_dev(e._h, src.data_ptr(), rb, d_keep.data_ptr(), n, dst.data_ptr()), "og_gate_gather_dev")
            e.sync()
            return (time.perf_counter() - t) / iters
        once(3)
        assert torch.equal(dst.view(n, rb)[::37], src.view(B, rb)[torch.from_numpy(keep[::37].astype(np.int64)).to("cuda:0")])
        gbs = [2 * n * rb / once(10) / 1e9 for _ in range(reps)]       # bytes read plus bytes written
        rows.append({"rows": n, "of": B, "row_bytes": rb, "path": "16 bytes per lane" if rb % 16 == 0 else "a byte per lane",
                     "gb_per_s": [round(v, 1) for v in gbs]})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    return rows


def child(precision, reps):
    import numpy as np

    import openglottal_amd as og
    from openglottal_amd import gated, synth
    from openglottal_amd.yolo import YoloV8Detector

    d = YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0", precision=precision)
    feats = (32, 64, 128, 256)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5))
    m.to("cuda:0").eval()
    if precision == "f16":
        m.set_option("precision", 2)
    e = gated.GatedEngine(m, d)
    e.set_params(max_shift_px=1e9, max_hold_frames=0)
    rows = []
    for n, h, w in SIZES:
        base = np.random.RandomState(h + w).randint(0, 256, (min(n, 100), h, w, 3), dtype=np.uint8)
        fr = np.tile(base, (-(-n // len(base)), 1, 1, 1))[:n]
        raw = d.detect_frames(base, 0.0)[:, 4]

        def run(conf, skip):
            e.reset()
            t = time.perf_counter()
            out = e.run(fr, conf=conf, want_boxes=False, skip_unboxed=skip)
            return time.perf_counter() - t, out

        for frac in FRACTIONS:
            conf = 0.0 if frac >= 1.0 else float(np.quantile(raw, 1.0 - frac))
            _, a = run(conf, False)                                           # warm-up of the plain engine
            t_first, b = run(conf, True)                                      # the first kept pass at this size and fraction
            assert np.array_equal(a["area"], b["area"])
            plain, kept = [], []
            for _ in range(reps):
                plain.append(n / run(conf, False)[0])
                kept.append(n / run(conf, True)[0])
            rows.append({"frames": n, "shape": [h, w], "precision": precision, "target_fraction": frac, "conf": conf,
                         "kept_fraction": round(b["kept"] / n, 3), "plain_fps": [round(v, 1) for v in plain], "kept_fps": [round(v, 1) for v in kept],
                         "first_kept_pass_fps": round(n / t_first, 1), "slowest_kept_over_fastest_plain": round(min(kept) / max(plain), 3),
                         "fastest_kept_over_slowest_plain": round(max(kept) / min(plain), 3),
                         "plain_spread": round(max(plain) / min(plain) - 1.0, 3)})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"rows": rows, "gather": gather_leg(e, reps) if precision == "f32" else []}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--precision", default="f32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.child:
        return child(a.precision, a.reps)
    rows, gather = [], []
    for p in ("f32", "f16"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--precision", p, "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, timeout=a.timeout)   # a fresh process; stderr passes through
        except subprocess.TimeoutExpired:
            print(f"{p}: time limit: stopping", file=sys.stderr)
            raise SystemExit(124)
        if r.returncode != 0:
            print(f"{p} ended with status {r.returncode}: stopping", file=sys.stderr)
            raise SystemExit(r.returncode)
        res = json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])
        rows += res["rows"]
        gather += res["gather"]
    summary = {"rows": rows, "gather": gather,
               "method": f"{a.reps} alternating repetitions after a warm-up, one process per precision; frames per second of "
                         "GatedEngine.run on pageable BGR frames, areas only, stage_kib 65536; the first kept pass (cold buffers and "
                         "graph cache) apart; slowest kept run over fastest plain run.  gather: GB/s read plus written by "
                         "k_gate_gather alone, 10 launches per figure"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
