#!/usr/bin/env python3
"""f16 mode ("precision" 2) against split precision ("precision" 1) of the SAME build on the SAME card in one call.

Starts `bench.py --full --no-parity --no-latency-mode --no-pipelines --no-cpu-baseline --option precision=N` (headline,
`host_inclusive`, `roofline` / `per_kernel_ms`) as fresh child processes, alternating N = 1, 2, 1, 2, 1, 2, one after the other,
each under its own time limit; stops at the first non-zero exit status.  Writes the JSON lines and a summary to
profiles/f16_vs_split.json (or --out).  bench.py itself is not touched.

bench.py's `roofline` block divides by the f32 MFMA peak for precision=2 (it knows only precision=1), so its `frac` is NOT the
number to read for this mode.  The summary recomputes, from the block's `achieved` TFLOP/s and `chain_ms`:
  * dominant kernel against the dense f16 MFMA peak (2 500 TFLOP/s; one MFMA per product in this mode, so no division by 3);
  * the chain's HBM fraction under the layer-boundary model at 2 bytes per element (91.8 MB per frame): frames of
    the profiled launch / chain_ms x 91.8 MB / 8 TB/s; and the same for the headline frames/s.

    python tools/bench_precision.py [--runs 3] [--steps 10] [--warmup 2] [--timeout 300] [--out FILE] [--f32]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_F16_MFMA_TFLOPS = 2500.0          # bench.py: PEAK_F16_MFMA_TFLOPS
PEAK_HBM_BYTES = 8.0e12                # bench.py: PEAK_HBM_BYTES
BYTES_PER_FRAME_2B = 91.8e6            # layer-boundary model at 16 bit


def run_once(options, steps, warmup, limit):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--full",
           "--no-parity", "--no-latency-mode", "--no-pipelines", "--no-cpu-baseline"]
    for o in options:
        cmd += ["--option", o]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, timeout=limit)      # a fresh process; stderr passes through
    if p.returncode != 0:
        return p.returncode, None
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    return 0, json.loads(lines[-1])


def brief(tag, r):
    rl = r.get("roofline") or {}
    out = {"leg": tag, "frames_per_s": r["value"], "host_inclusive": (r.get("host_inclusive") or {}).get("value"),
           "dominant_kernel": rl.get("kernel"), "dominant_achieved_tflops": rl.get("achieved"), "chain_ms": rl.get("chain_ms"),
           "frames_per_profiled_launch": rl.get("frames_per_launch"), "share_of_chain_time": rl.get("share_of_chain_time")}
    if tag == "f16" and rl:
        out["dominant_frac_of_f16_mfma_peak"] = round(rl["achieved"] / PEAK_F16_MFMA_TFLOPS, 4)
        out["chain_executed_frac_of_f16_mfma_peak"] = round(rl["chain"]["executed_tflops"] / PEAK_F16_MFMA_TFLOPS, 4)
        fps_chain = rl["frames_per_launch"] / (rl["chain_ms"] * 1e-3)
        out["one_lane_chain_frac_hbm_layer_boundary_2B"] = round(fps_chain * BYTES_PER_FRAME_2B / PEAK_HBM_BYTES, 4)
        out["headline_frac_hbm_layer_boundary_2B"] = round(r["value"] * BYTES_PER_FRAME_2B / PEAK_HBM_BYTES, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--f32", action="store_true", help="one more run without an option at the end: the f32 headline of this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_vs_split.json"))
    a = ap.parse_args()

    legs = [("split", ["precision=1"]), ("f16", ["precision=2"])] * a.runs + ([("f32", [])] if a.f32 else [])
    raw, rows = [], []
    for tag, opts in legs:
        try:
            rc, r = run_once(opts, a.steps, a.warmup, a.timeout)
        except subprocess.TimeoutExpired:
            rc, r = 124, None
        if rc != 0:
            print(f"bench.py {opts} ended with status {rc}: stopping", file=sys.stderr)
            raise SystemExit(rc)
        raw.append({"leg": tag, "options": opts, "result": r})
        rows.append(brief(tag, r))
        print(json.dumps(rows[-1]), flush=True)

    def vals(tag, key):
        return [x[key] for x in rows if x["leg"] == tag and x[key] is not None]

    f16, split, f32 = vals("f16", "frames_per_s"), vals("split", "frames_per_s"), vals("f32", "frames_per_s")
    f16h, splith = vals("f16", "host_inclusive"), vals("split", "host_inclusive")
    summary = {
        "frames_per_s": {"f16": f16, "split": split, "f32": f32},
        "host_inclusive": {"f16": f16h, "split": splith},
        "slowest_f16_over_fastest_split": round(min(f16) / max(split), 3),
        "median_f16_over_median_split": round(sorted(f16)[len(f16) // 2] / sorted(split)[len(split) // 2], 3),
        "host_inclusive_slowest_f16_over_fastest_split": round(min(f16h) / max(splith), 3) if f16h and splith else None,
        "f16_over_f32": round(sorted(f16)[len(f16) // 2] / f32[0], 3) if f32 else None,
        "slowest_f16_above_fastest_split": min(f16) > max(split) and (not f16h or min(f16h) > max(splith)),
        "f16_rows": [x for x in rows if x["leg"] == "f16"],
        "north_star_40pct_hbm_met": max(x.get("headline_frac_hbm_layer_boundary_2B", 0.0) for x in rows if x["leg"] == "f16") >= 0.40,
        "note": "bench.py's own roofline.frac divides by the f32 peak for precision=2: read the *_f16_mfma_peak / *_hbm_* fields here instead",
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"summary": summary, "runs": raw}, f, indent=1)
    print(json.dumps(summary))
    if not summary["slowest_f16_above_fastest_split"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
