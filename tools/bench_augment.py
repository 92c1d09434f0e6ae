#!/usr/bin/env python
"""The crop trainer's data path on the device: same build, same process, legs alternating over `--runs` runs
each, the slowest device run against the fastest host run.  Recorded, not a gate.

* workload: one epoch over 2 000 resident tiles at 256 x 256, batch 16, every sample augmented by its (seed, epoch, sample) record;
* legs: ``CropCacheLoader`` (device: four launches per batch, the records up, nothing down), the host twin on 16 threads, and the
  reference's chain restated in torch on the CPU (grid_sample, interpolate, conv2d, randn_like) on 16 threads of one sample each;
* the yardstick of what a training step can hide: the U-Net forward of one batch of 16 (``UNet.segment`` on 16 frames, u8 in, masks out).

    python tools/bench_augment.py --out profiles/augment_bench.json
"""
import argparse
import concurrent.futures
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from openglottal_amd import augment as A  # noqa: E402


def tiles(n, S, distinct=40):
    r = np.random.default_rng(0)
    y, x = np.mgrid[0:S, 0:S]
    base, masks = [], []
    for s in range(distinct):
        cy, cx = S * (0.4 + 0.2 * r.random()), S * (0.4 + 0.2 * r.random())
        img = 200 - 260 * np.hypot((y - cy) / S, (x - cx) / S) + 12 * np.sin(x / 9.0 + s) + r.normal(0, 2.0, (S, S))
        gap = np.abs(x - cx) < S * 0.03 * (1 + np.cos((y - cy) / S * 3))
        img[gap] *= 0.25
        base.append(img.clip(0, 255).astype(np.uint8))
        masks.append((gap & (np.abs(y - cy) < S * 0.3)).astype(np.uint8) * 255)
    return (np.stack([np.roll(base[i % distinct], i // distinct, axis=1) for i in range(n)]),
            np.stack([np.roll(masks[i % distinct], i // distinct, axis=1) for i in range(n)]))


def torch_sample(img, msk, v):
    """`_tensor_and_augment` with torchvision's functions restated in the torch functionals they reduce to (tests/aug_cases.py)"""
    import torch

    import aug_cases as AC

    S = img.shape[0]
    I = torch.from_numpy(img.astype(np.float32) / np.float32(255.0))
    M = torch.from_numpy((msk > 0).astype(np.float32))
    dims = [d for d, on in ((1, v["hflip"]), (0, v["vflip"])) if on]
    if dims:
        I, M = torch.flip(I, dims), torch.flip(M, dims)
    grid = AC.rotate_grid(S, v["angle"], torch.float32)
    I = torch.nn.functional.grid_sample(I[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    M = torch.nn.functional.grid_sample(M[None, None], grid, mode="nearest", padding_mode="zeros", align_corners=False)
    if v["new_size"]:
        n = v["new_size"]
        I = AC.fit(torch.nn.functional.interpolate(I, size=(n, n), mode="bilinear", align_corners=False, antialias=True), S)
        M = AC.fit(torch.nn.functional.interpolate(M, size=(n, n), mode="nearest"), S)
    if v["noise_sigma"]:
        I = torch.clamp(I + torch.randn_like(I) * v["noise_sigma"], 0.0, 1.0)
    if v["ks"]:
        k = torch.from_numpy(A.blur_kernel(v["ks"], v["blur_sigma"]))
        r = v["ks"] // 2
        I = torch.nn.functional.conv2d(torch.nn.functional.pad(I, [r, r, r, r], mode="reflect"), torch.mm(k[:, None], k[None, :])[None, None])
    if v["brightness"]:
        I = torch.clamp(I * v["brightness"], 0.0, 1.0)
    if v["contrast"]:
        I = torch.clamp(v["contrast"] * I + (1.0 - v["contrast"]) * I.mean(), 0.0, 1.0)
    return I[0], M[0]


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_bench.json"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=2000)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    a = ap.parse_args()
    import torch

    import openglottal_amd as og
    from openglottal_amd import synth

    torch.set_num_threads(1)                                                  # the pool's 16 threads take a sample each
    N, S, B = a.tiles, a.size, a.batch
    im, mk = tiles(N, S)
    dev = A.CropCacheLoader((im, mk), batch=B, seed=1, decode="device")
    pool = concurrent.futures.ThreadPoolExecutor(16)
    epoch = 0

    def device_epoch():
        dev.set_epoch(epoch)
        n = 0
        for imgs, _ in dev:
            n += imgs.shape[0]
        return n

    def twin_epoch():
        recs = [A.sample_record(1, epoch, n, S) for n in range(N)]
        return sum(o[0].shape[0] for o in pool.map(lambda n: A.augment_host(im[n:n + 1], mk[n:n + 1], [0], [recs[n]]), range(N)))

    def torch_epoch():
        vals = [A.draw_values(random.Random(A.sample_key(1, epoch, n, 1)), S) for n in range(N)]
        return sum(o[0].shape[0] for o in pool.map(lambda n: torch_sample(im[n], mk[n], vals[n]), range(N)))

    feats = (32, 64, 128, 256)
    model = og.UNet(1, 1, feats)
    model.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5))
    model.to("cuda:0").eval()
    frames = im[:B]

    def unet_steps():                                                         # as many forwards as the epoch has batches
        for _ in range(len(dev)):
            model.segment(frames, want_area=False)
        return N

    legs = {"device_loader": device_epoch, "twin_16_threads": twin_epoch, "torch_cpu_16_threads": torch_epoch, "unet_forward": unet_steps}
    device_epoch()                                                            # warm-up: workspace, pinned slots, the model's graphs
    unet_steps()
    times = {k: [] for k in legs}
    for r in range(a.runs):
        epoch = r
        for k, fn in legs.items():
            t, n = timed(fn)
            assert n == N
            times[k].append(t)
    pool.shutdown()
    batches = len(dev)
    res = {"tool": "tools/bench_augment.py", "runs": a.runs, "convention": "slowest device run over fastest host run, same build, same process",
           "tiles": N, "shape": [S, S], "batch": B, "batches_per_epoch": batches, "seconds_per_epoch": times,
           "ms_per_batch": {k: 1e3 * (max(v) if k in ("device_loader", "unet_forward") else min(v)) / batches for k, v in times.items()},
           "samples_per_second": {k: N / (max(v) if k in ("device_loader", "unet_forward") else min(v)) for k, v in times.items()}}
    for h in ("twin_16_threads", "torch_cpu_16_threads"):
        res[f"device_slowest_over_{h}_fastest"] = max(times["device_loader"]) / min(times[h])
    res["device_loader_over_unet_forward"] = max(times["device_loader"]) / min(times["unet_forward"])
    res["torch_cpu_16_threads_over_unet_forward"] = min(times["torch_cpu_16_threads"]) / max(times["unet_forward"])
    print(json.dumps(res["ms_per_batch"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
