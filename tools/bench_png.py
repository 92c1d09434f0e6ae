#!/usr/bin/env python
"""PNG files decoded on the device: same build, same process, legs alternating over `--runs` runs each, the
slowest device run against the fastest host run.  Recorded, not a gate.

* inputs: 2 000 Pillow-written 256 x 256 RGB files at level 6; 512 gray files at 480 x 640; a BAGLS-shaped mix of 3 500 files
  (256 x 256, 512 x 256, 512 x 128, 352 x 208; RGB frames and gray label masks);
* legs: ``PngDecoder.decode`` (parse, IDAT join, upload, the three kernels, pixels back) and ``decode_resident`` (pixels stay on
  the device), against a Pillow loop on one thread and on a 16-thread pool (Pillow releases the GIL while it decodes);
* per-kernel times (k_png_inflate, k_png_unfilter, k_png_expand) from a child process under
  ``rocprofv3 --kernel-trace --stats`` that decodes the first input once;
* ``evaluate_device`` over the BAGLS-shaped mix from files, both ways: ``png.read_pairs`` against the Pillow loop.

    python tools/bench_png.py --out profiles/png_bench.json
"""
import argparse
import concurrent.futures
import csv
import glob
import io
import json
import os
import shutil
import subprocess
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
    base[np.abs(x - cx) < W * 0.03 * (1 + np.cos((y - cy) / H * 3))] *= 0.25
    img = base[..., None] * np.array([1.0, 0.62, 0.55]) + r.normal(0, 2.0, (H, W, 3))
    img = img.clip(0, 255).astype(np.uint8)
    return img[..., 1] if gray else img


def mask(H, W, seed):
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    cy, cx = H * (0.4 + 0.2 * r.random()), W * (0.4 + 0.2 * r.random())
    return ((np.abs(x - cx) < W * 0.03 * (1 + np.cos((y - cy) / H * 3))) & (np.abs(y - cy) < H * 0.3)).astype(np.uint8) * 255


def png_bytes(a):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(a).save(b, "PNG", compress_level=6)
    return b.getvalue()


def cycle(base, n):
    return [base[i % len(base)] for i in range(n)]


def inputs(scale):
    n1, n2, n3 = max(8, int(2000 * scale)), max(8, int(512 * scale)), max(8, int(3500 * scale))
    yield "256x256 RGB level 6", cycle([png_bytes(picture(256, 256, s)) for s in range(32)], n1)
    yield "480x640 gray level 6", cycle([png_bytes(picture(480, 640, s, True)) for s in range(16)], n2)
    yield "BAGLS-shaped mix", bagls_mix(n3)[0]


def bagls_mix(n):
    """(files, image files, label files): n files, alternately a frame and its label mask, the four sizes in turn"""
    imgs, segs = [], []
    for i in range(16):
        H, W = BAGLS_SIZES[i % 4]
        imgs.append(png_bytes(picture(H, W, 100 + i)))
        segs.append(png_bytes(mask(H, W, 100 + i)))
    pairs = n // 2
    fi, fs = cycle(imgs, pairs), cycle(segs, pairs)
    return [f for p in zip(fi, fs) for f in p], fi, fs


def pillow_one(f):
    from PIL import Image

    im = Image.open(io.BytesIO(f))
    return np.asarray(im.convert("L" if im.mode in ("L", "1", "LA") else "RGB"))


def pillow_rgb(f):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))


def save(results, out):
    if out:
        with open(out, "w") as f:
            json.dump(results, f, indent=1)


def bench_decode(results, runs, scale, out, chunk=128):
    import torch

    d = P.PngDecoder(chunk)
    pool = concurrent.futures.ThreadPoolExecutor(16)
    for name, files in inputs(scale):
        n = len(files)
        k = min(n, 4)
        got = d.decode(files[:k])
        for g, f in zip(got, files[:k]):                                     # warm-up; device = twin = Pillow
            assert np.array_equal(g, P.decode_host(f)) and np.array_equal(g[..., ::-1], pillow_rgb(f))
        d.decode_resident(files[:k])
        t_dec, t_res, t_one, t_pool = [], [], [], []
        for _ in range(runs):                                                # legs alternating
            t = time.perf_counter()
            d.decode(files)
            t_dec.append(time.perf_counter() - t)
            torch.cuda.synchronize()
            t = time.perf_counter()
            d.decode_resident(files)
            torch.cuda.synchronize()
            t_res.append(time.perf_counter() - t)
            t = time.perf_counter()
            for f in files:
                pillow_one(f)
            t_one.append(time.perf_counter() - t)
            t = time.perf_counter()
            list(pool.map(pillow_one, files, chunksize=16))
            t_pool.append(time.perf_counter() - t)
        info = P.parse(files[0])
        rec = {"input": name, "files": n, "first_file": {k2: info[k2] for k2 in ("H", "W", "ctype", "depth")},
               "compressed_bytes_per_file": sum(len(f) for f in files) / n, "decode_s": t_dec, "decode_resident_s": t_res,
               "pillow_1_thread_s": t_one, "pillow_16_threads_s": t_pool,
               "files_per_s": {"decode_slowest": n / max(t_dec), "decode_resident_slowest": n / max(t_res), "pillow_1_thread_fastest": n / min(t_one),
                               "pillow_16_threads_fastest": n / min(t_pool)},
               "slowest_decode_over_fastest_pillow_1_thread": min(t_one) / max(t_dec),
               "slowest_decode_over_fastest_pillow_16_threads": min(t_pool) / max(t_dec),
               "slowest_decode_resident_over_fastest_pillow_1_thread": min(t_one) / max(t_res),
               "slowest_decode_resident_over_fastest_pillow_16_threads": min(t_pool) / max(t_res)}
        results["decode"].append(rec)
        save(results, out)
        print(json.dumps({k2: (round(v, 4) if isinstance(v, float) else v) for k2, v in rec.items() if not k2.endswith("_s")}), flush=True)


def bench_kernels(results, scale, out):
    """a fresh child under rocprofv3 decodes the first input once; the k_png_* rows of its kernel statistics"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    rec = {}
    if not os.path.exists(prof):
        rec["error"] = "rocprofv3 not found"
    else:
        with tempfile.TemporaryDirectory() as tmp:
            cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "png", "--", sys.executable, os.path.abspath(__file__),
                   "--only", "kernels-child", "--scale", str(scale)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired:
                r = subprocess.CompletedProcess(cmd, 124, "", "the profiled child took more than 300 s")
            rows = {}
            for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    name = row.get("Name", "")
                    if "k_png_" in name:
                        key = "k_png_" + name.split("k_png_")[1].split("(")[0]
                        rows[key] = {"calls": int(row.get("Calls", 0)), "total_ms": float(row.get("TotalDurationNs", 0)) / 1e6}
            if rows:
                rec.update(rows)
                rec["input"] = "256x256 RGB level 6, one decode_resident call after a warm-up call of 4 files"
            else:
                rec["error"] = f"no k_png_ rows (rocprofv3 exit {r.returncode}): {(r.stderr or r.stdout)[-300:]}"
    results["kernels"] = rec
    save(results, out)
    print(json.dumps({"kernels": rec}), flush=True)


def kernels_child(scale):
    name, files = next(inputs(scale))
    d = P.PngDecoder(chunk=1024)
    d.decode_resident(files[:4])
    d.decode_resident(files)


def bench_evaluate(results, runs, scale, out):
    """`evaluate_device` over the BAGLS-shaped mix, from files: png.read_pairs against the Pillow loop"""
    from PIL import Image

    import openglottal_amd as og
    from openglottal_amd import evaluate as E

    g = np.load(os.path.join(ROOT, "tests", "golden", "unet_trained_small.npz"))
    m = og.UNet(1, 1, tuple(int(f) for f in g["features"]))
    m.load_state_dict({k[2:]: g[k] for k in g.files if k.startswith("W:")})
    m.to("cuda:0").eval()
    _, imgs, segs = bagls_mix(max(8, int(3500 * scale)))
    d = P.PngDecoder()

    def device():
        frames, gts = P.read_pairs(imgs, segs, d)
        return E.evaluate_device(frames, gts, m)

    def host():
        frames = [np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))[..., ::-1]) for f in imgs]
        gts = [np.asarray(Image.open(io.BytesIO(f)).convert("L")) for f in segs]
        return E.evaluate_device(frames, gts, m)

    same = device() == host()                                                # warm-up, and the same aggregate
    t_dev, t_host = [], []
    for _ in range(runs):
        t = time.perf_counter()
        device()
        t_dev.append(time.perf_counter() - t)
        t = time.perf_counter()
        host()
        t_host.append(time.perf_counter() - t)
    rec = {"pairs": len(imgs), "aggregates_identical": bool(same), "read_pairs_then_evaluate_device_s": t_dev, "pillow_then_evaluate_device_s": t_host,
           "slowest_device_over_fastest_host": min(t_host) / max(t_dev)}
    results["evaluate_device"] = rec
    save(results, out)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["decode", "kernels", "kernels-child", "evaluate"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the file counts (a quick look)")
    ap.add_argument("--chunk", type=int, default=128, help="files per micro-batch of the decode legs (the handle's default: 128)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_png.py measures on the GPU: none found")
    if a.only == "kernels-child":
        return kernels_child(a.scale)
    results = {"card": torch.cuda.get_device_name(0), "day": time.strftime("%Y-%m-%d"), "runs": a.runs, "scale": a.scale, "chunk": a.chunk, "decode": []}
    if a.only in (None, "decode"):
        bench_decode(results, a.runs, a.scale, a.out, a.chunk)
    if a.only in (None, "kernels"):
        bench_kernels(results, a.scale, a.out)
    if a.only in (None, "evaluate"):
        bench_evaluate(results, a.runs, a.scale, a.out)
    save(results, a.out)


if __name__ == "__main__":
    main()
