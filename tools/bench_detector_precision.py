#!/usr/bin/env python3
"""The detector's f16 mode ("precision" 2) against its f32 path on the SAME build on the SAME card in one call.

Every measurement runs in a fresh child process, one after the other, each under its own time limit; the legs alternate
(f32, f16, f32, f16, ...) and the tool stops at the first non-zero exit status.

  * detector alone, 256 resident frames per launch (og_yolo_detect_u8_dev), f32 against f16, --runs each.  ACCEPTANCE: the slowest f16
    run is faster than the fastest f32 run (exit status 1 otherwise);
  * one-frame `detect` latency (`YoloV8Detector.__call__`, pageable frame in, box out), median of --calls calls, in the same children.
    f16 mode never splits K where the f32 latency path does; measured about equal.  Recorded, not a failure condition;
  * gated pipeline (tools/bench_gated.py, 2 000 frames, U-Net in f16), detector f32 against f16;
  * with --parent-lib FILE: the f32 detector of this build against the library built from the parent commit, alternating.

    python tools/bench_detector_precision.py [--runs 3] [--parent-lib FILE] [--out profiles/yolo_f16_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(precision, launches, calls):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from openglottal_amd import synth
    from openglottal_amd._lib import check, lib, ptr
    from openglottal_amd.yolo import YoloV8Detector

    d = YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0")
    if precision != "f32":   # (the parent commit's library knows no "precision": the f32 legs never set it)
        d.set_option("precision", 2)
    B = 256
    host = np.random.default_rng(0).integers(0, 256, (B, 256, 256, 3), dtype=np.uint8)
    bgr = torch.from_numpy(host).cuda()
    best = torch.empty((B, 5), dtype=torch.float32, device="cuda")

    def launch():
        check(lib().og_yolo_detect_u8_dev(d._h, ptr(bgr), B, 256, 256, 0.25, ptr(best), None), "og_yolo_detect_u8_dev")

    for _ in range(3):
        launch()
    check(lib().og_yolo_sync(d._h), "og_yolo_sync")
    t0 = time.perf_counter()
    for _ in range(launches):
        launch()
    check(lib().og_yolo_sync(d._h), "og_yolo_sync")
    fps = launches * B / (time.perf_counter() - t0)
    for i in range(20):
        d(host[i], 0.25)
    lat = []
    for i in range(calls):
        t = time.perf_counter()
        d(host[i % B], 0.25)
        lat.append(time.perf_counter() - t)
    lat.sort()
    print(json.dumps({"precision": precision, "frames_per_launch": B, "launches": launches, "frames_per_s": round(fps, 1),
                      "one_frame_detect_us_median": round(lat[len(lat) // 2] * 1e6, 1), "one_frame_detect_us_p90": round(lat[int(len(lat) * 0.9)] * 1e6, 1),
                      "best_head": best[:2].cpu().numpy().round(3).tolist()}))


def run_child(args, env_extra, limit):
    env = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable] + args, cwd=ROOT, stdout=subprocess.PIPE, timeout=limit, env=env)   # a fresh process; stderr passes through
    if p.returncode != 0:
        return p.returncode, None
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    return 0, json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["f32", "f16"])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--gated-frames", type=int, default=2000)
    ap.add_argument("--timeout", type=int, default=150, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libopenglottal_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolo_f16_bench.json"))
    a = ap.parse_args()
    if a.child:
        child(a.child, a.launches, a.calls)
        return

    me = [os.path.abspath(__file__), "--launches", str(a.launches), "--calls", str(a.calls)]
    legs = [("detector_" + p, me + ["--child", p], {}) for _ in range(a.runs) for p in ("f32", "f16")]
    gated = [os.path.join(ROOT, "tools", "bench_gated.py"), str(a.gated_frames)]
    legs += [("gated_unet_f16_detector_" + p, gated, {"OG_PRECISION": "2", "OG_DETECTOR_PRECISION": p}) for _ in range(2) for p in ("f32", "f16")]
    if a.parent_lib:
        lib_env = {"OPENGLOTTAL_HIP_LIB": os.path.abspath(a.parent_lib)}
        legs += [(t, me + ["--child", "f32"], e) for _ in range(a.runs) for t, e in (("parent_f32", lib_env), ("this_f32", {}))]
    rows = []
    for tag, args, env in legs:
        try:
            rc, r = run_child(args, env, a.timeout)
        except subprocess.TimeoutExpired:
            rc, r = 124, None
        if rc != 0:
            print(f"{tag} ended with status {rc}: stopping", file=sys.stderr)
            raise SystemExit(rc)
        rows.append({"leg": tag, "result": r})
        print(json.dumps(rows[-1]), flush=True)

    def vals(tag, key):
        return [x["result"][key] for x in rows if x["leg"] == tag]

    f32, f16 = vals("detector_f32", "frames_per_s"), vals("detector_f16", "frames_per_s")
    summary = {
        "detector_alone_frames_per_s": {"f32": f32, "f16": f16},
        "slowest_f16_over_fastest_f32": round(min(f16) / max(f32), 3),
        "median_f16_over_median_f32": round(sorted(f16)[len(f16) // 2] / sorted(f32)[len(f32) // 2], 3),
        "slowest_f16_above_fastest_f32": min(f16) > max(f32),
        "one_frame_detect_us_median": {"f32": vals("detector_f32", "one_frame_detect_us_median"), "f16": vals("detector_f16", "one_frame_detect_us_median")},
        "gated_2000_frames_unet_f16_fps": {"detector_f32": vals("gated_unet_f16_detector_f32", "fps"), "detector_f16": vals("gated_unet_f16_detector_f16", "fps")},
    }
    if a.parent_lib:
        pf, tf = vals("parent_f32", "frames_per_s"), vals("this_f32", "frames_per_s") + f32
        summary["f32_detector_parent_build_vs_this_build"] = {
            "parent": pf, "this": tf, "spreads_overlap": min(tf) <= max(pf) and min(pf) <= max(tf),
            "one_frame_us": {"parent": vals("parent_f32", "one_frame_detect_us_median"), "this": vals("this_f32", "one_frame_detect_us_median")}}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"summary": summary, "runs": rows}, f, indent=1)
    print(json.dumps(summary))
    if not summary["slowest_f16_above_fastest_f32"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
