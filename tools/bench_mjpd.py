#!/usr/bin/env python
"""Baseline JPEG decoded on the device: same build, same process, legs alternating, the spread shown, the
slowest device run against the fastest host run.  Recorded, not a gate.

* decode only, against the ``mjpeg.decode_jpeg_bgr`` loop (Pillow, one call per frame):
  2 000 frames at 256 x 256 from our encoder (4:4:4, Ri = 16, quality 75); 512 frames at 480 x 640 Pillow-encoded 4:2:0 without DRI
  (one lane per frame: the worst case) and with ``restart_marker_blocks=16``.  Two device legs: ``decode_resident`` (host bytes in:
  parse, upload of the compressed bytes, the four kernels) and ``decode_dev`` (everything resident: the kernels alone);
* end to end: `cli infer --pipeline unet-only --avi device --no-npy`'s block loop from an ``.avi``, ``--decode device`` against
  ``--decode host`` -- frames/s and bytes uploaded per frame.

Kernel times come from a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mjpd -- python tools/bench_mjpd.py --only decode --runs 1

    python tools/bench_mjpd.py --out profiles/mjpd_bench.json
"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_mjpeg import make_frames  # noqa: E402
from openglottal_amd import mjpeg as MJ  # noqa: E402


def pillow_files(n, H, W, restart, seed):
    from PIL import Image

    frames = make_frames(min(n, 16), H, W, seed)
    base = []
    for f in frames:
        b = io.BytesIO()
        kw = {"restart_marker_blocks": restart} if restart else {}
        Image.fromarray(np.ascontiguousarray(f[..., ::-1])).save(b, "JPEG", quality=75, subsampling=2, **kw)
        base.append(b.getvalue())
    return [base[i % len(base)] for i in range(n)]


def cases(scale):
    n1, n2 = max(4, int(2000 * scale)), max(4, int(512 * scale))
    own = [MJ.encode_host(f, 75) for f in make_frames(16, 256, 256, 3)]
    yield "256x256 own encoder 4:4:4 Ri=16 q75", [own[i % 16] for i in range(n1)]
    yield "480x640 Pillow 4:2:0 no DRI q75", pillow_files(n2, 480, 640, 0, 5)
    yield "480x640 Pillow 4:2:0 Ri=16 q75", pillow_files(n2, 480, 640, 16, 5)


def bench_decode(results, runs, scale, host_frames):
    import torch

    d = MJ.MjpegDecoder()
    for name, files in cases(scale):
        n = len(files)
        info = MJ.parse(files[0])
        H, W = info["H"], info["W"]
        k = min(n, 3)
        assert np.array_equal(d.decode(files[:k]), np.stack([MJ.decode_host(j) for j in files[:k]]))      # warm-up; device = twin
        assert np.array_equal(MJ.decode_host(files[0]), MJ.decode_jpeg_bgr(files[0]))                      # twin = Pillow
        blob, offsets, recs, tabs, form = MJ.records_host(files)
        d.set_tables(tabs, form["sampling"], form["Ri"])
        blob_d, off_d, recs_d = (torch.from_numpy(a).cuda() for a in (blob, offsets, recs))
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")
        d.decode_dev(blob_d, off_d, recs_d, n, H, W, out, out.numel(), status)
        d.sync()
        assert not status.any()
        nh = min(n, host_frames)
        t_res, t_dev, t_host = [], [], []
        for _ in range(runs):                                              # legs alternating
            torch.cuda.synchronize()
            t = time.perf_counter()
            d.decode_resident(files)
            t_res.append(time.perf_counter() - t)
            d.set_tables(tabs, form["sampling"], form["Ri"])
            torch.cuda.synchronize()
            t = time.perf_counter()
            d.decode_dev(blob_d, off_d, recs_d, n, H, W, out, out.numel(), status)
            d.sync()
            t_dev.append(time.perf_counter() - t)
            t = time.perf_counter()
            for j in files[:nh]:
                MJ.decode_jpeg_bgr(j)
            t_host.append((time.perf_counter() - t) / nh * n)             # scaled to the n frames of the device legs
        rec = {"case": name, "frames": n, "H": H, "W": W, "sampling": MJ.SAMPLING[info["sampling"]], "Ri": info["Ri"], "nI": info["nI"],
               "compressed_bytes_per_frame": sum(len(j) for j in files) / n, "decoded_bytes_per_frame": H * W * 3,
               "decode_resident_s": t_res, "decode_dev_s": t_dev, "host_loop_s_scaled_from_frames": nh, "host_loop_s": t_host,
               "decode_resident_fps_slowest": n / max(t_res), "decode_dev_fps_slowest": n / max(t_dev), "host_loop_fps_fastest": n / min(t_host),
               "speedup_slowest_decode_resident_over_fastest_host": min(t_host) / max(t_res),
               "speedup_slowest_decode_dev_over_fastest_host": min(t_host) / max(t_dev)}
        results["decode"].append(rec)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items() if not k.endswith("_s")}), flush=True)


def bench_end_to_end(results, runs, scale):
    """`cli infer --pipeline unet-only --avi device --no-npy`'s block loop at 256 x 256, from an .avi written by our own encoder"""
    import openglottal_amd as og
    from openglottal_amd import infer as I
    from openglottal_amd import synth

    feats = (32, 64, 128, 256)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5))
    m.to("cuda:0").eval()
    n, H, W = max(8, int(2000 * scale)), 256, 256
    own = [MJ.encode_host(f, 75) for f in make_frames(16, H, W, 7)]
    files = [own[i % 16] for i in range(n)]
    enc = MJ.Mjpeg()
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in.avi")
        with MJ.AviWriter(src, W, H) as w:
            w.write(np.frombuffer(b"".join(files), np.uint8), [len(j) for j in files])

        def run(decode):
            video = MJ.open_compressed(src) if decode == "device" else MJ.read_avi_mjpeg(src)
            up = video.compressed_bytes if decode == "device" else n * H * W * 3
            avi = MJ.AviWriter(os.path.join(tmp, f"{decode}.avi"), W, H, 25.0)
            for blob, sizes, _ in I.iter_pipeline_mjpeg(video, None, "unet-only", m, "cuda:0", encoder=enc):
                avi.write(blob, sizes)
            avi.close()
            return up

        run("device"), run("host")                                         # warm-up
        same = open(os.path.join(tmp, "device.avi"), "rb").read() == open(os.path.join(tmp, "host.avi"), "rb").read()
        t_new, t_old = [], []
        for _ in range(runs):
            t = time.perf_counter()
            up_new = run("device")
            t_new.append(time.perf_counter() - t)
            t = time.perf_counter()
            up_old = run("host")
            t_old.append(time.perf_counter() - t)
    rec = {"frames": n, "H": H, "W": W, "pipeline": "unet-only", "outputs_identical": same, "decode_device_s": t_new, "decode_host_s": t_old,
           "fps_device_slowest": n / max(t_new), "fps_host_fastest": n / min(t_old), "device_slowest_over_host_fastest": min(t_old) / max(t_new),
           "bytes_uploaded_per_frame_device": up_new / n, "bytes_uploaded_per_frame_host": up_old / n}
    results["end_to_end"] = rec
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items() if not k.endswith("_s")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["decode", "end-to-end"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (a quick look)")
    ap.add_argument("--host-frames", type=int, default=100, help="frames the host loop really decodes (its time is scaled)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mjpd.py measures on the GPU: none found")
    results = {"card": torch.cuda.get_device_name(0), "day": time.strftime("%Y-%m-%d"), "runs": a.runs, "scale": a.scale, "decode": []}
    if a.only in (None, "decode"):
        bench_decode(results, a.runs, a.scale, a.host_frames)
    if a.only in (None, "end-to-end"):
        bench_end_to_end(results, a.runs, a.scale)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
