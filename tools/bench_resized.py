#!/usr/bin/env python3
"""Frames that are not 256 x 256, measured in one process; prints one JSON line.

* `unet_segment_frame` ms per call (the reference's per-frame loop, features.py:234-238) at 256^2, 512^2 and 480x640: the device
  path (k_resize_in -> chain -> k_resize_out) and `unet_segment_frame_host` (numpy resizes and sigmoid around a device chain);
* frames/s of the streamed resized engine on BGR videos: `area_waveform` on a pageable array, and `UNet.segment_resized` on a
  pinned torch tensor (the same engine without the staging copy), at 256^2, 512^2, 480x640 and 1080x1920.

    python tools/bench_resized.py [--frames 2000] [--frames-hd 256] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import openglottal_amd as og  # noqa: E402
from openglottal_amd import synth  # noqa: E402
from openglottal_amd.features import area_waveform  # noqa: E402
from openglottal_amd.utils import unet_segment_frame, unet_segment_frame_host  # noqa: E402


def model():
    g = np.load(os.path.join(ROOT, "tests", "golden", "unet_trained_full.npz"))
    feats = tuple(int(f) for f in g["features"])
    sd = {k[2:]: (g[k].astype(np.float32) if g[k].dtype == np.float16 else g[k]) for k in g.files if k.startswith("W:")}
    m = og.UNet(1, 1, feats)
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    return m


def video(n, h, w):
    """n BGR frames at h x w: 8 distinct glottis frames repeated (the content does not change the work)."""
    g, _ = synth.glottis_frames(1, 8, h=h, w=w, seed=77)
    bgr = np.repeat(g[..., None], 3, axis=3)
    return np.ascontiguousarray(np.resize(bgr, (n, h, w, 3)))


def per_call(fn, frames, reps):
    for f in frames[:3]:
        fn(f)
    t0 = time.perf_counter()
    for i in range(reps):
        fn(frames[i % len(frames)])
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--frames-hd", type=int, default=256, help="frames of the 1080x1920 leg (2000 would be 12 GB of host memory)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    m = model()
    res = {"unit": {"per_call": "ms", "stream": "frames/s"}, "per_call": {}, "stream": {}}
    for h, w in ((256, 256), (512, 512), (480, 640)):
        g, _ = synth.glottis_frames(1, 8, h=h, w=w, seed=78)
        dev = per_call(lambda f: unet_segment_frame(f, m, None, 0.5), g, a.reps)
        host = per_call(lambda f: unet_segment_frame_host(f, m, None, 0.5), g, a.reps)
        res["per_call"][f"{h}x{w}"] = {"device": round(dev, 4), "host": round(host, 4)}
    for h, w in ((256, 256), (512, 512), (480, 640), (1080, 1920)):
        n = a.frames_hd if (h, w) == (1080, 1920) else a.frames
        v = video(n, h, w)
        area_waveform(v[:64], None, m)
        t0 = time.perf_counter()
        wave = area_waveform(v, None, m)
        pageable = n / (time.perf_counter() - t0)
        pinned_t = torch.from_numpy(v).pin_memory()
        m.segment_resized(pinned_t[:64], want_mask=False)
        t0 = time.perf_counter()
        _, area = m.segment_resized(pinned_t, want_mask=False)
        pinned = n / (time.perf_counter() - t0)
        assert np.array_equal(area.astype(np.float64), wave)
        res["stream"][f"{h}x{w}"] = {"frames": n, "area_waveform_pageable": round(pageable, 1), "segment_resized_pinned": round(pinned, 1),
                                     "host_link_GBps_pinned": round(pinned * h * w * 3 / 1e9, 2)}
        del pinned_t, v
    s256 = res["stream"]["256x256"]["area_waveform_pageable"]
    res["ratio_512_vs_256_area_waveform"] = round(res["stream"]["512x512"]["area_waveform_pageable"] / s256, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
