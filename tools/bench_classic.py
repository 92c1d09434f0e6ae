"""Recorded, not gated: the streamed guided-VFT pass (`classic.Classic.guided_vft`: upload, histograms, percentiles, threshold
recurrence, blob filter, areas on the device) against (a) the host composition of the same rules -- `og_bgr2gray_host` plus the
host twins, frame by frame -- and (b) the detector pass alone (the native YOLOv8n backend's batched `detect_frames`, random-init
weights), in the SAME build and the SAME process, over a seeded synthetic BGR video (`synth.bench_frame_bgr`) with scripted boxes at a
70 % detection rate.  The legs alternate, five runs each; reported: slowest device run over fastest run of the other leg.

    python tools/bench_classic.py [--frames 2000] [--runs 5] [--out profiles/classic_bench.json]

A second leg records what the frame size limit rests on: the blob filter's worst case (a one-pixel spiral, its transpose, a
serpentine, nested rings), one frame per launch, climbing 32, 64, 128, 256 and stopping before a side predicted to exceed 2 s.

    python tools/bench_classic.py --worst-case [--out profiles/classic_blobs_worst_case.json]

Frames above 65 536 pixels go through the tiled blob filter (include/openglottal_hip_classic_tiled.h): ``--size HxW`` sets the frame
size of the streamed leg and ``--tiled`` takes the handle's mode ("auto" when given without a value).  With ``--tiled always`` at a
size the one-workgroup filter also takes, a second device leg runs the same video with "off" in the same process, next to the
first, their order alternating from run to run.  ``--worst-case
--tiled`` climbs the same ladder on the tiled path, past 256 by doubling up to og_classic_tiled_limit(0), and times the
one-workgroup filter next to it up to 256.  Tiled runs are merged, one key per run, into profiles/classic_tiled.json.

    python tools/bench_classic.py --size 480x640 --tiled [--frames 500]
    python tools/bench_classic.py --size 1080x1920 --tiled --frames 100
    python tools/bench_classic.py --size 256x256 --tiled always
    python tools/bench_classic.py --worst-case --tiled
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scripted_boxes(n, h, w, rate=0.7, seed=2024):
    import numpy as np

    rs = np.random.RandomState(seed)
    boxes = []
    for _ in range(n):
        hit, bw, bh, cx, cy = rs.rand() < rate, rs.randint(48, w // 2), rs.randint(48, h // 2), rs.rand(), rs.rand()
        x1, y1 = int(cx * (w - bw)), int(cy * (h - bh))
        boxes.append((x1, y1, x1 + bw, y1 + bh) if hit else None)
    return boxes


def merge_into(out_path, key, rec):
    """profiles/classic_tiled.json holds one record per run of a tiled leg: replace this run's key, keep the others."""
    doc = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            doc = json.load(f)
    doc[key] = rec
    with open(out_path, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")


def worst_case_tiled(out_path):
    """worst_case() on the tiled path: the ladder's sides, then 512 and upward, doubling to og_classic_tiled_limit(0), with the same
    prediction rule; up to 256 the one-workgroup filter is timed on the same masks in the same process."""
    import datetime

    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import classic_cases as K
    from openglottal_amd import classic as CL
    from openglottal_amd._lib import lib

    limit, tile = int(lib().og_classic_tiled_limit(0)), int(lib().og_classic_tiled_limit(1))
    sides, S = list(K.LADDER_SIDES), 512
    while S * S <= limit:
        sides.append(S)
        S *= 2
    eng = {}
    for mode in ("always", "off"):
        eng[mode] = CL.Classic(beta=1.0, percentile=30, n_components=2, tiled=mode)
        eng[mode].thresh = 128.0
    rows, times, stopped = [], [], None
    for S in sides:
        if times and K.ladder_prediction(times) > K.LADDER_LIMIT_S:
            stopped = {"S": S, "predicted_s": round(K.ladder_prediction(times), 3)}
            break
        rung = []
        for name, m in K.ladder_masks(S):
            frames = torch.from_numpy(np.where(m > 0, 0, 255).astype(np.uint8)[None]).cuda()
            bx = torch.tensor([[0, 0, S, S]], dtype=torch.int32).cuda()
            out = torch.zeros((1, S, S), dtype=torch.uint8, device="cuda")
            area = torch.zeros((1,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            want_mask, want_area = CL.blobs_host(m, 2)
            row = {"mask": name, "S": S}
            for mode in ("always", "off") if S * S <= lib().og_classic_limit(0) else ("always",):
                took = []
                for _ in range(4):
                    t0 = time.perf_counter()
                    eng[mode].guided_vft_dev(frames, 1, S, S, 1, bx, area, out, None)
                    eng[mode].sync()
                    took.append(time.perf_counter() - t0)
                assert int(area.cpu()[0]) == want_area and np.array_equal(out.cpu().numpy()[0], want_mask), f"device and host twin disagree: {name} {S} {mode}"
                row["ms" if mode == "always" else "one_workgroup_ms"] = round(float(np.median(took[1:])) * 1e3, 4)
                if mode == "always":
                    row["warm_ms"] = round(took[0] * 1e3, 4)
                    rung.append(float(np.median(took[1:])))
            rows.append(row)
        times.append(max(rung))
    rec = {"kernels": "k_tblob_* (tiled, ms) next to k_blobs<1> (one_workgroup_ms)", "tile": tile, "limit_pixels": limit,
           "launch": "B=1, gray, box=frame, n=2, mask requested; wall clock around sync, median of 3 after a warm call",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "date": datetime.date.today().isoformat(), "limit_s": K.LADDER_LIMIT_S, "not_launched": stopped, "rungs": rows}
    print(json.dumps(rec), flush=True)
    merge_into(out_path, "worst_case", rec)
    return 1 if stopped else 0


def worst_case(out_path):
    """The worst case of k_blobs' labelling, timed smallest first (the masks, the sides, the prediction rule and the 2 s bound of
    tests/classic_cases.py, as tests/test_gpu_classic_blobs.py climbs them): one frame per launch through the resident entry, gray,
    box = frame, n = 2, mask requested; wall clock around the handle's sync, one warm call, the median of three.  A side whose
    predicted time exceeds the bound is not launched, and the record says so."""
    import datetime

    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import classic_cases as K
    from openglottal_amd import classic as CL

    e = CL.Classic(beta=1.0, percentile=30, n_components=2)
    e.thresh = 128.0
    rows, times, stopped = [], [], None
    for S in K.LADDER_SIDES:
        if times and K.ladder_prediction(times) > K.LADDER_LIMIT_S:
            stopped = {"S": S, "predicted_s": round(K.ladder_prediction(times), 3)}
            break
        rung = []
        for name, m in K.ladder_masks(S):
            frames = torch.from_numpy(np.where(m > 0, 0, 255).astype(np.uint8)[None]).cuda()
            bx = torch.tensor([[0, 0, S, S]], dtype=torch.int32).cuda()
            out = torch.zeros((1, S, S), dtype=torch.uint8, device="cuda")
            area = torch.zeros((1,), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            took = []
            for _ in range(4):
                t0 = time.perf_counter()
                e.guided_vft_dev(frames, 1, S, S, 1, bx, area, out, None)
                e.sync()
                took.append(time.perf_counter() - t0)
            want_mask, want_area = CL.blobs_host(m, 2)
            assert int(area.cpu()[0]) == want_area and np.array_equal(out.cpu().numpy()[0], want_mask), f"device and host twin disagree: {name} {S}"
            rung.append(float(np.median(took[1:])))
            rows.append({"mask": name, "S": S, "ms": round(rung[-1] * 1e3, 4), "warm_ms": round(took[0] * 1e3, 4)})
        times.append(max(rung))
    rec = {"kernel": "k_blobs<1>", "launch": "B=1, gray, box=frame, n=2, mask requested; wall clock around sync, median of 3 after a warm call",
           "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "date": datetime.date.today().isoformat(), "limit_s": K.LADDER_LIMIT_S, "not_launched": stopped, "rungs": rows}
    print(json.dumps(rec), flush=True)
    with open(out_path, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    return 1 if stopped else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-detector", action="store_true", help="skip leg (b)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--worst-case", action="store_true",
                    help="time the labelling's worst case instead (spiral, serpentine, rings at 32..256); writes --out, "
                         "default profiles/classic_blobs_worst_case.json")
    ap.add_argument("--size", default="256x256", help="HxW of the streamed leg's frames (above 256x256 needs --tiled)")
    ap.add_argument("--tiled", nargs="?", const="auto", default=None, choices=["off", "auto", "always"],
                    help="the handle's tiled mode; results are merged into profiles/classic_tiled.json (or --out)")
    a = ap.parse_args()
    tiled_out = a.out or os.path.join(ROOT, "profiles", "classic_tiled.json")
    if a.worst_case and a.tiled:
        sys.exit(worst_case_tiled(tiled_out))
    if a.worst_case:
        sys.exit(worst_case(a.out or os.path.join(ROOT, "profiles", "classic_blobs_worst_case.json")))

    import numpy as np

    from openglottal_amd import classic as CL
    from openglottal_amd import synth

    n = a.frames
    h, w = (int(v) for v in a.size.lower().split("x"))
    modes = [a.tiled or "off"]
    if a.tiled == "always" and h * w <= 65536:
        modes.append("off")                      # the one-workgroup filter on the same video, alternating
    video = np.stack([synth.bench_frame_bgr(i, h, w) for i in range(n)])
    boxes = scripted_boxes(n, h, w)
    engs = {m: CL.Classic(tiled=m) for m in modes}
    eng = engs[modes[0]]
    seed = eng.init(video[:2], boxes[0])

    def device(mode=modes[0]):
        engs[mode].thresh = seed
        return engs[mode].guided_vft(video, boxes, want_mask=False)[1]

    def host():
        return CL.guided_vft_host(video, boxes, seed)[1]

    detect = None
    if not a.no_detector:
        from openglottal_amd.yolo import YoloV8Detector

        det = YoloV8Detector(synth.make_yolov8_state_dict(seed=7))
        detect = lambda: det.detect_frames(video, 0.25)
    want = host()
    assert np.array_equal(device(), want), "device and host composition disagree"
    if detect:
        detect()
    t_dev, t_host, t_det, t_other = [], [], [], []
    for run in range(a.runs):
        t0 = time.perf_counter()
        r_host = host()
        took = {}
        for m in (modes if run % 2 == 0 else modes[::-1]):     # two device legs: adjacent, their order alternating from run to run
            t1 = time.perf_counter()
            r_dev = device(m)
            took[m] = time.perf_counter() - t1
            assert np.array_equal(r_dev, want), "device and host composition disagree"
        t2 = time.perf_counter()
        if detect:
            detect()
        t3 = time.perf_counter()
        assert np.array_equal(r_host, want), "device and host composition disagree"
        t_host.append(t2 - t0 - sum(took.values()))
        t_dev.append(took[modes[0]])
        if len(modes) > 1:
            t_other.append(took[modes[1]])
        t_det.append(t3 - t2)
    fps = lambda ts: [round(n / t, 1) for t in ts]
    row = {"frames": n, "shape": [h, w, 3], "detection_rate": round(sum(b is not None for b in boxes) / n, 3),
           "mean_area": round(float(want.mean()), 1), "host_composition_fps": fps(t_host), "device_fps": fps(t_dev),
           "slowest_device_over_fastest_host": round(min(fps(t_dev)) / max(fps(t_host)), 3)}
    if a.tiled:
        row["tiled"] = modes[0]
    if t_other:
        row["device_fps_" + modes[1]] = fps(t_other)
        row["slowest_" + modes[0] + "_over_fastest_" + modes[1]] = round(min(fps(t_dev)) / max(fps(t_other)), 3)
    if detect:
        row["detector_alone_fps"] = fps(t_det)
        row["slowest_device_over_fastest_detector"] = round(min(fps(t_dev)) / max(fps(t_det)), 3)
    print(json.dumps(row), flush=True)
    if a.tiled:
        merge_into(tiled_out, f"stream_{h}x{w}_{modes[0]}", row)
    elif a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
