#!/usr/bin/env python
"""Baseline JPEG on the device: same build, same process, legs alternating, five runs each, the spread shown,
slowest-new against fastest-old.  Recorded, not a gate.

* encoder alone: ``Mjpeg.encode_dev`` on 2 000 resident frames at 256 x 256 and 100 at 1080 x 1920 -- frames/s and bytes/frame;
* end to end: `cli infer`'s block loop with ``--avi device --no-npy`` (``iter_pipeline_mjpeg`` + ``AviWriter``) against the loop as
  it stood before (``iter_pipeline`` + ``NpyWriter``) on the same frames -- frames/s, bytes brought back per frame, bytes on disk;
* against the host twin: ``og_jpeg_encode_host`` over (a stated number of) the same frames.

Kernel times come from a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mjpeg -- python tools/bench_mjpeg.py --only encoder --runs 1
    python tools/bench_mjpeg.py --kernel-stats DIR/.../mjpeg_kernel_stats.csv --merge profiles/mjpeg_bench.json

The second command adds, per kernel, its time and its share of its roof: the larger of bytes over the HBM copy rate and 32-bit vector
operations over the vector rate, both counted from the shapes by ``kernel_model`` below, over the measured time.

    python tools/bench_mjpeg.py --out profiles/mjpeg_bench.json
"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openglottal_amd import mjpeg as MJ  # noqa: E402

HBM_COPY_TBS = 6.29          # measured float4 copy on an MI355X (8.0 TB/s spec)
VALU_TOPS = 256 * 64 * 2.4e9 / 1e12      # 32-bit vector operations per second at one per lane and clock: 256 CUs x 64 lanes x 2.4 GHz
CASES = ((2000, 256, 256), (100, 1080, 1920))


def make_frames(n, H, W, seed):
    """annotated-looking frames: a smooth gray scene with sensor noise, a green outline and fill, a yellow box; 16 distinct ones, shifted"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = []
    for i in range(16):
        g = 110 + 60 * np.sin(xx / (W / 6.0) + i) * np.cos(yy / (H / 4.0)) + rs.normal(0, 4, (H, W))
        f = np.repeat(np.clip(g, 0, 255).astype(np.uint8)[..., None], 3, 2)
        d = ((yy - H / 2) / (H / 5.0)) ** 2 + ((xx - W / 2 - 3 * i) / (W / 14.0)) ** 2
        f[d < 1.0, 1] = np.minimum(255, f[d < 1.0, 1].astype(int) + 102).astype(np.uint8)
        f[(d < 1.0) & (d > 0.9)] = (0, 255, 0)
        y0, y1, x0, x1 = H // 4, 3 * H // 4, W // 3, 2 * W // 3
        f[[y0, y1], x0:x1] = (0, 220, 255)
        f[y0:y1, [x0, x1]] = (0, 220, 255)
        base.append(f)
    return np.stack([np.roll(base[i % 16], i // 16, axis=1) for i in range(n)])


def kernel_model(n, H, W, total_bytes):
    """bytes moved and 32-bit vector operations per kernel for n frames, from the shapes (a multiply-add is one operation)"""
    M = ((H + 7) // 8) * ((W + 7) // 8)
    nI = (M + MJ.limit(1) - 1) // MJ.limit(1)
    scan = total_bytes - n * (MJ.limit(6) + 2)
    return {
        # reads the frame once, writes 384 bytes per MCU; per MCU 64 x 15 colour operations, 2 x 3 x 8 x 64 multiply-adds, 192 divisions of ~20
        "k_mjpeg_transform": {"bytes": n * (H * W * 3 + M * 384), "ops": n * M * (64 * 15 + 3072 + 192 * 20)},
        # reads the coefficients, writes the interval's bytes; two walks over 192 coefficients per MCU at ~8 operations each, a walk over the bytes
        "k_mjpeg_entropy": {"bytes": n * (M * 384 + nI * 4) + scan, "ops": n * M * 192 * 2 * 8 + scan * 6},
        "k_mjpeg_offsets": {"bytes": n * nI * 12, "ops": n * nI * 4},
        "k_mjpeg_place": {"bytes": 2 * total_bytes + n * nI * 12, "ops": total_bytes * 2},
    }


def roof_share(model, seconds):
    t_bytes, t_ops = model["bytes"] / (HBM_COPY_TBS * 1e12), model["ops"] / (VALU_TOPS * 1e12)
    return {"least_s": max(t_bytes, t_ops), "roof": "HBM bytes" if t_bytes >= t_ops else "vector operations",
            "share_of_roof": max(t_bytes, t_ops) / seconds}


def bench_encoder(results, runs, scale, host_frames):
    import torch

    e = MJ.Mjpeg()
    for n, H, W in CASES:
        n = max(1, int(n * scale))
        frames = make_frames(n, H, W, seed=H)
        dev = torch.from_numpy(frames).cuda()
        cap = n * MJ.bound(H, W)
        out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        sizes = torch.empty(n, dtype=torch.int32, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        k = min(n, 4)
        blob, sz = e.encode(frames[:k])                                    # the warm-up, and the device against the twin
        assert blob.tobytes() == b"".join(MJ.encode_host(f, e.quality) for f in frames[:k])
        e.encode_dev(dev, n, H, W, out, cap, sizes, total)
        e.sync()
        nh = min(n, host_frames)
        res, host = [], []
        for _ in range(runs):                                              # legs alternating
            torch.cuda.synchronize()
            t = time.perf_counter()
            e.encode_dev(dev, n, H, W, out, cap, sizes, total)
            e.sync()
            res.append(time.perf_counter() - t)
            t = time.perf_counter()
            for f in frames[:nh]:
                MJ.encode_host(f, e.quality)
            host.append((time.perf_counter() - t) / nh * n)               # scaled to the n frames of the device leg
        tot = int(total.item())
        rec = {"frames": n, "H": H, "W": W, "quality": e.quality, "bytes_per_frame": tot / n, "source_bytes_per_frame": H * W * 3,
               "encode_dev_s": res, "host_twin_s_scaled_from_frames": nh, "host_twin_s": host,
               "encode_dev_fps_slowest": n / max(res), "encode_dev_fps_fastest": n / min(res),
               "host_twin_fps_fastest": n / min(host), "speedup_slowest_device_over_fastest_host": min(host) / max(res),
               "kernel_model": kernel_model(n, H, W, tot)}
        results["encoder"].append(rec)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items() if not k.endswith("_s") and k != "kernel_model"}),
              flush=True)


def bench_end_to_end(results, runs, scale):
    """`cli infer --pipeline unet-only`'s block loop at 256 x 256, written to a scratch directory"""
    import torch  # noqa: F401

    import openglottal_amd as og
    from openglottal_amd import infer as I
    from openglottal_amd import synth

    feats = (32, 64, 128, 256)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5))
    m.to("cuda:0").eval()
    n, H, W = max(8, int(2000 * scale)), 256, 256
    frames = make_frames(n, H, W, seed=7)
    enc = MJ.Mjpeg()
    with tempfile.TemporaryDirectory() as d:
        def new():
            avi, back = None, 0
            for blob, sizes, area in I.iter_pipeline_mjpeg(frames, None, "unet-only", m, "cuda:0", encoder=enc):
                avi = avi or MJ.AviWriter(os.path.join(d, "new.avi"), W, H, 25.0)
                avi.write(blob, sizes)
                back += blob.nbytes + sizes.nbytes + 4 * len(sizes)
            avi.close()
            return back, os.path.getsize(os.path.join(d, "new.avi"))

        def old():
            w, back = I.NpyWriter(os.path.join(d, "old.npy"), n), 0
            for blk, area in I.iter_pipeline(frames, None, "unet-only", m, "cuda:0"):
                w.write(blk)
                back += blk.nbytes + 4 * len(blk)
            w.close()
            return back, os.path.getsize(os.path.join(d, "old.npy"))

        new(), old()                                                       # warm-up
        t_new, t_old = [], []
        for _ in range(runs):
            t = time.perf_counter()
            b_new, disk_new = new()
            t_new.append(time.perf_counter() - t)
            t = time.perf_counter()
            b_old, disk_old = old()
            t_old.append(time.perf_counter() - t)
    rec = {"frames": n, "H": H, "W": W, "pipeline": "unet-only", "avi_device_no_npy_s": t_new, "iter_pipeline_npy_writer_s": t_old,
           "fps_new_slowest": n / max(t_new), "fps_old_fastest": n / min(t_old), "new_slowest_over_old_fastest": min(t_old) / max(t_new),
           "bytes_back_per_frame_new": b_new / n, "bytes_back_per_frame_old": b_old / n, "bytes_on_disk_new": disk_new,
           "bytes_on_disk_old": disk_old}
    results["end_to_end"] = rec
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items() if not k.endswith("_s")}), flush=True)


def merge_kernel_stats(path, stats_csv):
    """per kernel: total time of the traced run (one warm-up call of 4 frames, then 1 + runs calls per case) and its share of roof"""
    with open(path) as f:
        results = json.load(f)
    rows = {}
    with open(stats_csv, newline="") as f:
        for r in csv.DictReader(f):
            for k in ("k_mjpeg_transform", "k_mjpeg_entropy", "k_mjpeg_offsets", "k_mjpeg_place"):
                if k in r["Name"]:
                    rows[k] = {"calls": int(r["Calls"]), "total_s": int(r["TotalDurationNs"]) / 1e9}
    calls = results.get("traced_runs", 1) + 1                              # encode_dev calls per case in the traced run
    model = {k: {"bytes": 0, "ops": 0} for k in rows}
    for c in results["encoder"]:
        for k in rows:
            model[k]["bytes"] += calls * c["kernel_model"][k]["bytes"]
            model[k]["ops"] += calls * c["kernel_model"][k]["ops"]
    results["kernels"] = {k: {**rows[k], **model[k], **roof_share(model[k], rows[k]["total_s"])} for k in rows}
    results["kernels_note"] = ("time over both cases of the traced run (the 4-frame warm-up calls are in the time and not in the model: below 1 %); "
                               f"roofs: {HBM_COPY_TBS} TB/s HBM copy, {VALU_TOPS:.1f} T 32-bit vector operations/s")
    with open(path, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results["kernels"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["encoder", "end-to-end"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (a quick look)")
    ap.add_argument("--host-frames", type=int, default=20, help="frames the host twin's leg really codes (its time is scaled)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of `--only encoder --runs R`")
    ap.add_argument("--traced-runs", type=int, default=1, help="the R of that run")
    ap.add_argument("--merge", default=None, help="the JSON of an earlier --out to add the kernel figures to")
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.merge) as f:
            r = json.load(f)
        r["traced_runs"] = a.traced_runs
        with open(a.merge, "w") as f:
            json.dump(r, f, indent=1)
        return merge_kernel_stats(a.merge, a.kernel_stats)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mjpeg.py measures on the GPU: none found")
    results = {"card": torch.cuda.get_device_name(0), "day": time.strftime("%Y-%m-%d"), "runs": a.runs, "scale": a.scale,
               "hbm_copy_TBs": HBM_COPY_TBS, "valu_Tops": VALU_TOPS, "encoder": []}
    if a.only in (None, "encoder"):
        bench_encoder(results, a.runs, a.scale, a.host_frames)
    if a.only in (None, "end-to-end"):
        bench_end_to_end(results, a.runs, a.scale)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
