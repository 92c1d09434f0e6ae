#!/usr/bin/env python3
"""The gated pipeline (`features.area_waveform` with a detector): the device engine of DESIGN section 16 (`engine="device"`: one upload
per frame, detector, tracker and U-Net in one device pass) against the staged pass (`engine="staged"`: detector on a worker
thread, the state machine in Python, a second upload for the U-Net) on the SAME build, in the SAME process, on one card.

Recorded, not gated: the tool always exits 0 when every leg ran.  One child process per precision, under its own time limit, one
after the other.  Inside a child, per frame size, the two legs alternate (staged, engine, staged, engine, ...) after a warm-up,
--reps times each; a row reports every run and the SLOWEST engine run over the FASTEST staged run.  Input: seeded noise frames (100
distinct frames, tiled) in pageable memory; the boxes are the detector's own output on them at its default confidence.

    python tools/bench_gated_engine.py [--reps 5] [--out profiles/gated_engine.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((2000, 256, 256), (512, 480, 640), (64, 1080, 1920))


def child(precision, reps, stage_kib):
    import numpy as np

    import openglottal_amd as og
    from openglottal_amd import features, gated, synth
    from openglottal_amd.yolo import YoloV8Detector

    d = YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0", precision=precision)
    feats = (32, 64, 128, 256)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5))
    m.to("cuda:0").eval()
    if precision == "f16":
        m.set_option("precision", 2)
    rows = []
    for n, h, w in SIZES:
        base = np.random.RandomState(h + w).randint(0, 256, (min(n, 100), h, w, 3), dtype=np.uint8)
        fr = np.tile(base, (-(-n // len(base)), 1, 1, 1))[:n]

        def run(engine):
            det = og.TemporalDetector(d)
            if stage_kib and engine == "device":
                features.gated_engine_for(fr, det, m, policy=False).set_option("stage_kib", stage_kib)
            t = time.perf_counter()
            wave = features.area_waveform(fr, det, m, engine=engine)
            return time.perf_counter() - t, wave

        p0 = gated.GatedEngine.passes
        (_, a), (_, b) = run("staged"), run("device")     # warm-up (arenas, rings, slots) and the waveform
        assert np.array_equal(a, b) and gated.GatedEngine.passes == p0 + 1
        run("auto")                                       # which of the two does the default take at this size?
        auto = "engine" if gated.GatedEngine.passes == p0 + 2 else "staged"
        staged, eng = [], []
        for _ in range(reps):
            staged.append(n / run("staged")[0])
            eng.append(n / run("device")[0])
        rows.append({"frames": n, "shape": [h, w], "precision": precision, "staged_fps": [round(v, 1) for v in staged],
                     "engine_fps": [round(v, 1) for v in eng], "slowest_engine_over_fastest_staged": round(min(eng) / max(staged), 3),
                     "fastest_engine_over_slowest_staged": round(max(eng) / min(staged), 3), "frames_with_area": int((a > 0).sum()), "auto_takes": auto})
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"rows": rows}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--precision", default="f32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stage-kib", type=int, default=0, help="the engine's micro-batch setting (0: its default, 65536)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gated_engine.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.child:
        return child(a.precision, a.reps, a.stage_kib)
    rows = []
    for p in ("f32", "f16"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--precision", p, "--reps", str(a.reps), "--stage-kib", str(a.stage_kib)]
        try:
            r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, timeout=a.timeout)   # a fresh process; stderr passes through
        except subprocess.TimeoutExpired:
            print(f"{p}: time limit: stopping", file=sys.stderr)
            raise SystemExit(124)
        if r.returncode != 0:
            print(f"{p} ended with status {r.returncode}: stopping", file=sys.stderr)
            raise SystemExit(r.returncode)
        rows += json.loads([l for l in r.stdout.decode().splitlines() if l.startswith("{")][-1])["rows"]
    summary = {"rows": rows, "stage_kib": a.stage_kib or 65536,
               "method": f"{a.reps} alternating repetitions after a warm-up, one process per precision; frames per second of "
                         "features.area_waveform on pageable BGR frames; slowest engine run over fastest staged run"}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
