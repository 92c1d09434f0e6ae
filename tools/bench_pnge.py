#!/usr/bin/env python
"""PNG files encoded on the device: same build, same process, legs alternating over `--runs` runs each, the
slowest device run against the fastest host run.  Recorded, not a gate.

* workloads: 2 000 annotated-looking RGB frames at 256 x 256; 512 gray frames at 480 x 640; 2 000 crop tile + mask pairs at 256 x 256;
* legs: ``PngEncoder.encode`` (frames up, the four kernels, files back), ``encode_resident`` with the files fetched (frames already on
  the device: what `cli infer --png device` and `cropcache.build` do), against a Pillow loop on one thread and on a 16-thread pool, at
  Pillow's default compression and at ``compress_level=1``;
* the bytes per frame that cross the bus, each way;
* `cli infer --no-npy --avi device --frames png --png device` against the same command with Pillow's files (which needs the .npy);
* ``cropcache.build`` (ground-truth ROI) on 2 000 mixed-size pairs, device against its host twin.

    python tools/bench_pnge.py --out profiles/pnge_bench.json
"""
import argparse
import concurrent.futures
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from openglottal_amd import png as P  # noqa: E402

BAGLS_SIZES = [(256, 256), (512, 256), (512, 128), (352, 208)]


def picture(H, W, seed, gray=False):
    """an endoscope-like frame: smooth shading, a dark gap, sensor noise"""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    cy, cx = H * (0.4 + 0.2 * r.random()), W * (0.4 + 0.2 * r.random())
    d = np.hypot((y - cy) / H, (x - cx) / W)
    base = 200 - 260 * d + 12 * np.sin(x / 9.0 + seed) + 10 * np.cos(y / 13.0)
    gap = np.abs(x - cx) < W * 0.03 * (1 + np.cos((y - cy) / H * 3))
    base[gap] *= 0.25
    img = base[..., None] * np.array([1.0, 0.62, 0.55]) + r.normal(0, 2.0, (H, W, 3))
    img = img.clip(0, 255).astype(np.uint8)
    m = (gap & (np.abs(y - cy) < H * 0.3)).astype(np.uint8) * 255
    return (img[..., 1] if gray else img), m


def stack(n, H, W, gray, distinct=40):
    """n frames from `distinct` pictures, each shifted a little: different bytes, the same statistics"""
    base = [picture(H, W, s, gray) for s in range(distinct)]
    return np.stack([np.roll(base[i % distinct][0], i // distinct, axis=1) for i in range(n)]), \
        np.stack([np.roll(base[i % distinct][1], i // distinct, axis=1) for i in range(n)])


def pillow_file(f, level):
    from PIL import Image

    b = io.BytesIO()
    im = Image.fromarray(np.ascontiguousarray(f[..., ::-1]) if f.ndim == 3 else f)
    if level is None:
        im.save(b, "PNG")
    else:
        im.save(b, "PNG", compress_level=level)
    return b.getvalue()


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def bench_workload(name, frames, runs):
    import torch

    B = len(frames)
    C = 3 if frames.ndim == 4 else 1
    H, W = frames.shape[1:3]
    enc = P.PngEncoder()
    dev = torch.from_numpy(frames).cuda()
    pool = concurrent.futures.ThreadPoolExecutor(16)
    legs = {
        "device_streamed": lambda: sum(len(f) for f in enc.files(frames)),
        "device_resident": lambda: sum(len(f) for f in enc.files_resident(dev, B, H, W, C)),
        "pillow_1_thread": lambda: sum(len(pillow_file(f, None)) for f in frames),
        "pillow_16_threads": lambda: sum(len(b) for b in pool.map(lambda f: pillow_file(f, None), frames)),
        "pillow_level1_1_thread": lambda: sum(len(pillow_file(f, 1)) for f in frames),
        "pillow_level1_16_threads": lambda: sum(len(b) for b in pool.map(lambda f: pillow_file(f, 1), frames)),
    }
    legs["device_streamed"]()                                                # warm-up: workspace and pinned slots
    legs["device_resident"]()
    times, sizes = {k: [] for k in legs}, {}
    for _ in range(runs):
        for k, fn in legs.items():
            t, n = timed(fn)
            times[k].append(t)
            sizes[k] = n
    pool.shutdown()
    res = {"frames": B, "shape": [H, W, C], "seconds": times, "file_bytes_per_frame": {k: v / B for k, v in sizes.items()},
           "bus_bytes_per_frame": {"device_streamed": {"up": H * W * C, "down": sizes["device_streamed"] / B},
                                   "device_resident": {"up": 0, "down": sizes["device_resident"] / B},
                                   "pillow": {"down": H * W * C}}}
    for d in ("device_streamed", "device_resident"):
        for h in [k for k in legs if k.startswith("pillow")]:
            res[f"{d}_slowest_over_{h}_fastest"] = max(times[d]) / min(times[h])
    res["frames_per_second"] = {k: B / (max(v) if k.startswith("device") else min(v)) for k, v in times.items()}
    print(name, json.dumps({k: round(v, 1) for k, v in res["frames_per_second"].items()}), flush=True)
    return res


def bench_infer(runs, n=512):
    import torch

    from openglottal_amd import cli, synth

    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        feats = (32, 64, 128, 256)
        torch.save(synth.state_dict_to_torch(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5)), os.path.join(tmp, "unet.pt"))
        os.makedirs(os.path.join(tmp, "in"))
        np.save(os.path.join(tmp, "in", "clip.npy"), stack(n, 256, 256, False)[0])
        base = ["infer", "--input", os.path.join(tmp, "in"), "--mode", "npy", "--pipeline", "unet-only", "--unet-weights", os.path.join(tmp, "unet.pt"),
                "--frames", "png", "--avi", "device"]
        legs = {"png_device_no_npy": ["--png", "device", "--no-npy"], "png_pillow": []}
        times = {k: [] for k in legs}
        stdout = sys.stdout
        for r in range(runs + 1):                                            # the first round warms everything up
            for k, extra in legs.items():
                sys.stdout = io.StringIO()
                try:
                    t, _ = timed(lambda: cli.main(base + ["--output-dir", os.path.join(tmp, k)] + extra))
                finally:
                    sys.stdout = stdout
                if r:
                    times[k].append(t)
        out = {"frames": n, "seconds": times, "device_slowest_over_pillow_fastest": max(times["png_device_no_npy"]) / min(times["png_pillow"])}
    print("cli infer", json.dumps(out["seconds"]), flush=True)
    return out


def bench_cropcache(runs, n=2000):
    from PIL import Image

    from openglottal_amd import cropcache

    with tempfile.TemporaryDirectory() as tmp:
        r = np.random.default_rng(1)
        ips, lps = [], []
        base = {s: [picture(s[1], s[0], k) for k in range(8)] for s in BAGLS_SIZES}
        for i in range(n):
            img, m = base[BAGLS_SIZES[int(r.integers(4))]][i % 8]
            ips.append(os.path.join(tmp, f"{i}.png"))
            lps.append(os.path.join(tmp, f"{i}_seg.png"))
            Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(ips[-1])
            Image.fromarray(m).save(lps[-1])
        times = {"device": [], "host": []}
        for rr in range(runs + 1):
            for where in ("device", "host"):
                if where == "host" and rr > 1:
                    continue                                                 # the twin is slow and steady: one timed run
                t, res = timed(lambda: cropcache.build(ips, lps, os.path.join(tmp, where), "train", roi="gt", decode=where, encode=where))
                if rr:
                    times[where].append(t)
        out = {"pairs": n, "kept": res["n"], "seconds": times, "device_slowest_over_host_fastest": max(times["device"]) / min(times["host"])}
    print("cropcache", json.dumps(out["seconds"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnge_bench.json"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the workloads' frame counts")
    a = ap.parse_args()
    n = lambda v: max(8, int(v * a.scale))   # noqa: E731
    res = {"tool": "tools/bench_pnge.py", "runs": a.runs, "convention": "slowest device run over fastest host run, same build, same process"}
    rgb, _ = stack(n(2000), 256, 256, False)
    res["rgb_256"] = bench_workload("rgb_256", rgb, a.runs)
    gray, _ = stack(n(512), 480, 640, True)
    res["gray_480x640"] = bench_workload("gray_480x640", gray, a.runs)
    tiles, masks = stack(n(2000), 256, 256, True)
    tiles[:, :40] = 0                                                         # letterbox padding
    masks[:, :40] = 0
    res["crop_tiles"] = bench_workload("crop_tiles", tiles, a.runs)
    res["crop_masks"] = bench_workload("crop_masks", masks, a.runs)
    res["cli_infer"] = bench_infer(a.runs, n(512))
    res["cropcache"] = bench_cropcache(a.runs, n(2000))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
