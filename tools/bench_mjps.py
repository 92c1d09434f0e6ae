#!/usr/bin/env python
"""Split entropy decode by tools/bench_mjpd.py's protocol: same build, same process, legs alternating, a warm-up
of every leg, a device synchronise around each leg, the spread shown, the slowest split run against the fastest run without it.
Recorded, not a gate.

* 512 frames at 480 x 640, Pillow 4:2:0, quality 75, WITHOUT DRI: split off (the lane per frame: what the decoder did before the mode
  existed, that path is untouched) and split on at sub 32, 64, 128 and 256; the same frames with ``restart_marker_blocks=16``, split
  off: the yardstick of what intervals give; 2 000 frames at 256 x 256 without DRI, on (the default sub) and off.
  Two timed legs per setting, as in bench_mjpd.py: ``decode_dev`` (everything resident: the kernels alone) and ``decode_resident``
  (host bytes in).  Before anything is timed every leg's bytes are compared: all equal, and equal to the host twin's on the first files.
* the rounds the twin counts (``og_jpegs_decode_host``'s stats) over the distinct files, per sub;
* `cli infer --pipeline unet-only --decode device` on the 480 x 640 .avi without DRI, with and without ``--decode-split auto``.

Kernel times come from a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mjps -- python tools/bench_mjps.py --only decode --runs 1

    python tools/bench_mjps.py --out profiles/mjps_bench.json
"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_mjpd import pillow_files  # noqa: E402
from openglottal_amd import mjpeg as MJ  # noqa: E402

SUBS = (32, 64, 128, 256)


def settings(case):
    """`(label, split, sub)` per leg of a case."""
    if case == "big":
        return [("off", "off", None)] + [(f"sub{s}", "auto", s) for s in SUBS]
    if case == "ri16":
        return [("off", "off", None)]
    return [("off", "off", None), ("default", "auto", None)]


def cases(scale):
    n1, n2 = max(4, int(2000 * scale)), max(4, int(512 * scale))
    yield "big", "480x640 Pillow 4:2:0 no DRI q75", pillow_files(n2, 480, 640, 0, 5)
    yield "ri16", "480x640 Pillow 4:2:0 Ri=16 q75", pillow_files(n2, 480, 640, 16, 5)
    yield "small", "256x256 Pillow 4:2:0 no DRI q75", pillow_files(n1, 256, 256, 0, 3)


def twin_rounds(files, subs):
    """per sub: lanes per file, mean and most rounds per window, decodes per lane -- over the distinct files"""
    out = {}
    distinct = list(dict.fromkeys(files))
    for sub in subs:
        rows = [MJ.decode_split_host(j, sub, 256, statuses=True, stats=True)[2] for j in distinct]
        lanes, windows = sum(r["lanes"] for r in rows), sum(r["windows"] for r in rows)
        out[str(sub)] = {"files": len(rows), "lanes_per_file": lanes / len(rows), "windows_per_file": windows / len(rows),
                         "most_rounds_of_a_window_mean_over_files": sum(r["rounds"] for r in rows) / len(rows),
                         "most_rounds_of_a_window": max(r["rounds"] for r in rows), "decodes_per_lane": sum(r["decodes"] for r in rows) / lanes}
    return out


def bench_decode(results, runs, scale):
    import torch

    for key, name, files in cases(scale):
        n = len(files)
        info = MJ.parse(files[0])
        H, W = info["H"], info["W"]
        legs = settings(key)
        decoders = {label: MJ.MjpegDecoder(split=split, sub=sub) for label, split, sub in legs}
        blob, offsets, recs, tabs, form = MJ.records_host(files)
        blob_d, off_d, recs_d = (torch.from_numpy(a).cuda() for a in (blob, offsets, recs))
        out = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        status = torch.zeros(n, dtype=torch.int32, device="cuda")

        def dev(d):
            d.set_tables(tabs, form["sampling"], form["Ri"])
            torch.cuda.synchronize()
            t = time.perf_counter()
            d.decode_dev(blob_d, off_d, recs_d, n, H, W, out, out.numel(), status)
            d.sync()
            return time.perf_counter() - t

        def resident(d):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = d.decode_resident(files)
            return time.perf_counter() - t, r

        # identical bytes first (this is the warm-up too): every leg, both entries, against the first leg; the twin on the first files
        want = None
        for label, d in decoders.items():
            dev(d)
            assert not status.any(), label
            got = out.clone()
            _, res = resident(d)
            assert torch.equal(res, got), label
            want = got if want is None else want
            assert torch.equal(got, want), f"{name}: leg {label} gives other bytes than leg off"
            del res
        k = min(n, 3)
        assert np.array_equal(want[:k].cpu().numpy(), np.stack([MJ.decode_host(j) for j in files[:k]]))
        t_dev, t_res = {label: [] for label in decoders}, {label: [] for label in decoders}
        for _ in range(runs):                                                  # legs alternating
            for label, d in decoders.items():
                t_dev[label].append(dev(d))
                t_res[label].append(resident(d)[0])
        rec = {"case": name, "frames": n, "H": H, "W": W, "sampling": MJ.SAMPLING[info["sampling"]], "Ri": info["Ri"],
               "compressed_bytes_per_frame": sum(len(j) for j in files) / n, "bytes_identical_across_legs": True, "legs": {}}
        for label, split, sub in legs:
            rec["legs"][label] = {"split": split, "sub": sub if sub else (MJ.split_limit(0) if split == "auto" else None),
                                  "decode_dev_s": t_dev[label], "decode_resident_s": t_res[label],
                                  "decode_dev_fps_slowest": n / max(t_dev[label]), "decode_dev_fps_fastest": n / min(t_dev[label]),
                                  "decode_resident_fps_slowest": n / max(t_res[label]), "decode_resident_fps_fastest": n / min(t_res[label])}
        on = [label for label, split, _ in legs if split == "auto"]
        if on:
            best = max(on, key=lambda label: rec["legs"][label]["decode_dev_fps_slowest"])
            rec["best_split_leg_by_slowest_run"] = best
            rec["slowest_split_over_fastest_off_decode_dev"] = min(t_dev["off"]) / max(t_dev[best])
            rec["slowest_split_over_fastest_off_decode_resident"] = min(t_res["off"]) / max(t_res[best])
            rec["twin_rounds"] = twin_rounds(files, SUBS if key == "big" else (MJ.split_limit(0),))
        results["decode"].append(rec)
        show = {k2: v for k2, v in rec.items() if k2 not in ("legs", "twin_rounds")}
        show["decode_dev_fps_slowest"] = {label: round(v["decode_dev_fps_slowest"], 1) for label, v in rec["legs"].items()}
        show["decode_resident_fps_slowest"] = {label: round(v["decode_resident_fps_slowest"], 1) for label, v in rec["legs"].items()}
        print(json.dumps(show), flush=True)
        if "twin_rounds" in rec:
            print(json.dumps(rec["twin_rounds"]), flush=True)


def bench_cli(results, runs, scale):
    """`cli infer --pipeline unet-only --decode device` on a 480 x 640 .avi without DRI, with and without `--decode-split auto`"""
    import torch

    from openglottal_amd import cli, synth

    feats = (32, 64, 128, 256)
    n = max(8, int(512 * scale))
    files = pillow_files(n, 480, 640, 0, 5)
    with tempfile.TemporaryDirectory() as tmp:
        torch.save(synth.state_dict_to_torch(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5)), os.path.join(tmp, "unet.pt"))
        os.makedirs(os.path.join(tmp, "in"))
        with MJ.AviWriter(os.path.join(tmp, "in", "clip.avi"), 640, 480) as w:
            w.write(np.frombuffer(b"".join(files), np.uint8), [len(j) for j in files])
        base = ["infer", "--input", os.path.join(tmp, "in"), "--pipeline", "unet-only", "--unet-weights", os.path.join(tmp, "unet.pt"), "--decode", "device"]

        def run(split):
            torch.cuda.synchronize()
            t = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                assert cli.main(base + ["--output-dir", os.path.join(tmp, split), "--decode-split", split]) == 0
            torch.cuda.synchronize()
            return time.perf_counter() - t

        run("off"), run("auto")                                            # warm-up
        same = all(open(os.path.join(tmp, "off", f), "rb").read() == open(os.path.join(tmp, "auto", f), "rb").read()
                   for f in sorted(os.listdir(os.path.join(tmp, "off"))))
        t_on, t_off = [], []
        for _ in range(runs):
            t_off.append(run("off"))
            t_on.append(run("auto"))
    rec = {"frames": n, "H": 480, "W": 640, "pipeline": "unet-only", "outputs_identical": same, "split_off_s": t_off, "split_auto_s": t_on,
           "fps_split_auto_slowest": n / max(t_on), "fps_split_off_fastest": n / min(t_off), "split_auto_slowest_over_off_fastest": min(t_off) / max(t_on)}
    results["cli_infer"] = rec
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in rec.items() if not k.endswith("_s")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["decode", "cli"], default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the frame counts (a quick look)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_mjps.py measures on the GPU: none found")
    results = {"card": torch.cuda.get_device_name(0), "day": time.strftime("%Y-%m-%d"), "runs": a.runs, "scale": a.scale,
               "default_sub": MJ.split_limit(0), "decode": []}
    if a.only in (None, "decode"):
        bench_decode(results, a.runs, a.scale)
    if a.only in (None, "cli"):
        bench_cli(results, a.runs, a.scale)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
