"""Recorded, not gated: the streamed guided-VFT pass (`classic.Classic.guided_vft`: upload, histograms, percentiles, threshold
recurrence, blob filter, areas on the device) against (a) the host composition of the same rules -- `og_bgr2gray_host` plus the
host twins, frame by frame -- and (b) the detector pass alone (the native YOLOv8n backend's batched `detect_frames`, random-init
weights), in the SAME build and the SAME process, over a seeded synthetic BGR video (`synth.bench_frame_bgr`) with scripted boxes at a
70 % detection rate.  The legs alternate, five runs each; reported: slowest device run over fastest run of the other leg.

    python tools/bench_classic.py [--frames 2000] [--runs 5] [--out profiles/classic_bench.json]

A second leg records what the frame size limit rests on: the blob filter's worst case (a one-pixel spiral, its transpose, a
serpentine, nested rings), one frame per launch, climbing 32, 64, 128, 256 and stopping before a side predicted to exceed 2 s.

    python tools/bench_classic.py --worst-case [--out profiles/classic_blobs_worst_case.json]
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
    a = ap.parse_args()
    if a.worst_case:
        sys.exit(worst_case(a.out or os.path.join(ROOT, "profiles", "classic_blobs_worst_case.json")))

    import numpy as np

    from openglottal_amd import classic as CL
    from openglottal_amd import synth

    n, h, w = a.frames, 256, 256
    video = np.stack([synth.bench_frame_bgr(i, h, w) for i in range(n)])
    boxes = scripted_boxes(n, h, w)
    eng = CL.Classic()
    seed = eng.init(video[:2], boxes[0])

    def device():
        eng.thresh = seed
        return eng.guided_vft(video, boxes, want_mask=False)[1]

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
    t_dev, t_host, t_det = [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        r_host = host()
        t1 = time.perf_counter()
        r_dev = device()
        t2 = time.perf_counter()
        if detect:
            detect()
        t3 = time.perf_counter()
        assert np.array_equal(r_host, want) and np.array_equal(r_dev, want), "device and host composition disagree"
        t_host.append(t1 - t0)
        t_dev.append(t2 - t1)
        t_det.append(t3 - t2)
    fps = lambda ts: [round(n / t, 1) for t in ts]
    row = {"frames": n, "shape": [h, w, 3], "detection_rate": round(sum(b is not None for b in boxes) / n, 3),
           "mean_area": round(float(want.mean()), 1), "host_composition_fps": fps(t_host), "device_fps": fps(t_dev),
           "slowest_device_over_fastest_host": round(min(fps(t_dev)) / max(fps(t_host)), 3)}
    if detect:
        row["detector_alone_fps"] = fps(t_det)
        row["slowest_device_over_fastest_detector"] = round(min(fps(t_dev)) / max(fps(t_det)), 3)
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
