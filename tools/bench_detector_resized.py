#!/usr/bin/env python3
"""The detector on frames of any size: the device letterbox (`detect_frames`, k_letterbox_bgr around the unchanged network) against
the host letterbox (`detect_frames_host`: `letterbox_bgr` per frame in numpy) on the SAME build, in the SAME process, on one card.

Every part runs in a child process under its own time limit, one after the other; the tool stops at the first non-zero exit status.
Inside a child the two paths alternate (host, device, host, device, ...) after a warm-up, --reps times each, and a row reports the
SLOWEST device run against the FASTEST host run.

  1. throughput: 512 pageable BGR frames at 480x640, 512 at 512x256, 64 at 1080x1920; f32 and f16;
  2. the one-frame call (`YoloV8Detector.__call__`, pageable frame in, box out): median of --calls calls, --reps medians, at
     480x640 (host composition, device with the source copied to the device, device with the source read from mapped pinned
     memory) and at 256x256, where the letterbox is the identity and the path must not have moved: with --parent-lib FILE the
     same figure is taken with the parent commit's library and the parent commit's `__call__`, alternating with this build's;
  3. gated `area_waveform`, 2 000 frames at 480x640: `detect_frames` against `detect_frames = detect_frames_host`.

ACCEPTANCE (exit status 1 otherwise): in no row of parts 1-3 is the slowest device run slower than the fastest host run, and the
256x256 call's median of medians is not above the parent's run-to-run spread (two parent processes, before and after).

    python tools/bench_detector_resized.py [--reps 5] [--parent-lib FILE] [--out profiles/yolo_resized_bench.json]

The per-kernel share comes from a separate run (one child, nothing else traced):
    rocprofv3 --kernel-trace --stats -- python tools/bench_detector_resized.py --child profile
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("og_yolo_letterbox_geometry", "og_yolo_letterbox_host", "og_yolo_letterbox_u8_dev", "og_yolo_detect_resized_u8",
               "og_yolo_detect_resized_u8_dev", "og_yolo_detect_resized_u8_begin", "og_yolo_launch_count")


def detector(precision):
    from openglottal_amd import synth
    from openglottal_amd.yolo import YoloV8Detector

    return YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0", precision=precision)


def noise(n, h, w):
    import numpy as np

    return np.random.RandomState(h + w).randint(0, 256, (n, h, w, 3), dtype=np.uint8)


def timed(fn):
    t = time.perf_counter()
    r = fn()
    return time.perf_counter() - t, r


def child_throughput(precision, reps):
    import numpy as np

    d = detector(precision)
    rows = []
    for n, h, w in ((512, 480, 640), (512, 512, 256), (64, 1080, 1920)):
        fr = noise(n, h, w)
        ref, got = d.detect_frames_host(fr[:8]), d.detect_frames(fr)     # warm-up (arena, stage) and the bits
        assert np.array_equal(got[:8].view(np.uint32), ref.view(np.uint32))
        host, dev = [], []
        for _ in range(reps):
            host.append(n / timed(lambda: d.detect_frames_host(fr))[0])
            dev.append(n / timed(lambda: d.detect_frames(fr))[0])
        rows.append({"frames": n, "shape": [h, w], "precision": precision, "host_fps": [round(v, 1) for v in host],
                     "device_fps": [round(v, 1) for v in dev], "slowest_device_over_fastest_host": round(min(dev) / max(host), 2),
                     "hits": int((got[:, 4] >= 0).sum())})
    print(json.dumps({"rows": rows}))


def median_us(fn, calls):
    lat = sorted(timed(fn)[0] for _ in range(calls))
    return round(lat[len(lat) // 2] * 1e6, 1)


def child_latency(precision, reps, calls, parent):
    import numpy as np

    if parent:   # the parent commit's library exports none of the new symbols; its `__call__` is today's detect_frames_host with B = 1
        from openglottal_amd import _lib
        for k in NEW_SYMBOLS:
            _lib.PROTOTYPES.pop(k)
    d = detector(precision)
    sq = noise(32, 256, 256)
    k = [0]

    def nxt(a):
        k[0] += 1
        return a[k[0] % len(a)]

    if parent:
        for _ in range(30):
            d.detect_frames_host(nxt(sq)[None])
        print(json.dumps({"precision": precision, "parent_call_256x256_us": [median_us(lambda: d.detect_frames_host(nxt(sq)[None]), calls) for _ in range(reps)]}))
        return
    big = noise(32, 480, 640)
    legs = {"call_256x256_us": lambda: d(nxt(sq)), "host_480x640_us": lambda: d.detect_frames_host(nxt(big)[None]),
            "device_480x640_source_copied_us": lambda: d(nxt(big)), "device_480x640_source_mapped_us": lambda: d(nxt(big))}
    out = {n: [] for n in legs}
    for _ in range(30):
        d(nxt(sq)), d(nxt(big))
    for _ in range(reps):
        for name, fn in legs.items():
            d.set_option("source_mapped", 1 if name.endswith("mapped_us") else 0)
            for _ in range(5):
                fn()
            out[name].append(median_us(fn, calls))
    d.set_option("source_mapped", 1)   # (the default)
    out["precision"] = precision
    print(json.dumps(out))


def child_gated(reps, n_frames):
    import numpy as np

    import openglottal_amd as og
    from openglottal_amd import features, synth

    d = detector("f32")
    feats = (32, 64, 128, 256)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5))
    m.to("cuda:0").eval()
    fr = np.tile(noise(100, 480, 640), (n_frames // 100, 1, 1, 1))

    def run(host):
        if host:
            d.detect_frames = d.detect_frames_host
        try:
            return features.area_waveform(fr, og.TemporalDetector(d), m)
        finally:
            if host:
                del d.detect_frames

    a, b = run(True), run(False)     # warm-up, and the waveform
    assert np.array_equal(a, b)
    host, dev = [], []
    for _ in range(reps):
        host.append(len(fr) / timed(lambda: run(True))[0])
        dev.append(len(fr) / timed(lambda: run(False))[0])
    print(json.dumps({"frames": len(fr), "shape": [480, 640], "host_letterbox_fps": [round(v, 1) for v in host], "device_letterbox_fps": [round(v, 1) for v in dev],
                      "slowest_device_over_fastest_host": round(min(dev) / max(host), 2)}))


def child_profile():
    d = detector("f32")
    fr = noise(512, 480, 640)
    for _ in range(3):
        d.detect_frames(fr)
    big = noise(64, 1080, 1920)
    for _ in range(3):
        d.detect_frames(big)
    for i in range(50):
        d(fr[i])
    print(json.dumps({"profiled": "3 x 512 frames 480x640, 3 x 64 frames 1080x1920, 50 one-frame calls 480x640"}))


def run_child(args, env_extra, limit):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, cwd=ROOT, stdout=subprocess.PIPE, timeout=limit,
                       env=dict(os.environ, **env_extra))   # a fresh process; stderr passes through
    if p.returncode != 0:
        return p.returncode, None
    return 0, json.loads([l for l in p.stdout.decode().splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["throughput", "latency", "gated", "profile"])
    ap.add_argument("--precision", default="f32")
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--gated-frames", type=int, default=2000)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    ap.add_argument("--parent-lib", default=None, help="libopenglottal_hip.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolo_resized_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    if a.child == "throughput":
        return child_throughput(a.precision, a.reps)
    if a.child == "latency":
        return child_latency(a.precision, a.reps, a.calls, a.parent)
    if a.child == "gated":
        return child_gated(a.reps, a.gated_frames)
    if a.child == "profile":
        return child_profile()

    common = ["--reps", str(a.reps), "--calls", str(a.calls), "--gated-frames", str(a.gated_frames)]
    legs = [("throughput_" + p, ["--child", "throughput", "--precision", p], {}) for p in ("f32", "f16")]
    for p in ("f32", "f16"):
        if a.parent_lib:
            legs.append(("latency_parent_" + p, ["--child", "latency", "--parent", "--precision", p], {"OPENGLOTTAL_HIP_LIB": os.path.abspath(a.parent_lib)}))
        legs.append(("latency_" + p, ["--child", "latency", "--precision", p], {}))
        if a.parent_lib:   # a second parent run: the parent's own run-to-run spread, in the same session
            legs.append(("latency_parent_again_" + p, ["--child", "latency", "--parent", "--precision", p], {"OPENGLOTTAL_HIP_LIB": os.path.abspath(a.parent_lib)}))
    legs.append(("gated", ["--child", "gated"], {}))
    res = {}
    for tag, args, env in legs:
        try:
            rc, r = run_child(args + common, env, a.timeout * (2 if tag == "gated" else 1))   # (the host baseline of part 3 is slow)
        except subprocess.TimeoutExpired:
            rc, r = 124, None
        if rc != 0:
            print(f"{tag} ended with status {rc}: stopping", file=sys.stderr)
            raise SystemExit(rc)
        res[tag] = r
        print(json.dumps({tag: r}), flush=True)

    rows = res["throughput_f32"]["rows"] + res["throughput_f16"]["rows"]
    ok = all(r["slowest_device_over_fastest_host"] >= 1.0 for r in rows) and res["gated"]["slowest_device_over_fastest_host"] >= 1.0
    one = {}
    for p in ("f32", "f16"):
        l = res["latency_" + p]
        ok = ok and max(l["device_480x640_source_copied_us"] + l["device_480x640_source_mapped_us"]) <= min(l["host_480x640_us"])
        one[p] = {k: v for k, v in l.items() if k != "precision"}
        if a.parent_lib:
            par = res["latency_parent_" + p]["parent_call_256x256_us"] + res["latency_parent_again_" + p]["parent_call_256x256_us"]
            one[p]["parent_call_256x256_us"] = par
            one[p]["parent_spread_us"] = [min(par), max(par)]   # two parent processes, one before and one after this build's
            one[p]["call_256x256_not_above_parent_spread"] = sorted(l["call_256x256_us"])[len(l["call_256x256_us"]) // 2] <= max(par)
            ok = ok and one[p]["call_256x256_not_above_parent_spread"]
    summary = {"throughput": rows, "one_frame_call": one, "gated_area_waveform": res["gated"], "device_never_slower_than_host": ok,
               "method": f"{a.reps} alternating repetitions after a warm-up; slowest device run over fastest host run; one-frame: medians of {a.calls} calls"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(summary, f, indent=1)
    print(json.dumps(summary))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
