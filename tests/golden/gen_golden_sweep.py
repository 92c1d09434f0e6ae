#!/usr/bin/env python3
"""Generate tests/golden/sweep_traces.json by RUNNING THE REFERENCE (build container only, as tests/golden/gen_golden.py)::

    python tests/golden/gen_golden_sweep.py

What is executed is the reference's own code, unmodified: `openglottal.models.detector.TemporalDetector.detect` behind the scripted
fake YOLO and the placeholder modules of gen_golden.py, once per (conf, max_hold_frames) over ONE script of about 120 frames, and
`frame_metrics` of `scripts/sweep_bagls_conf.py` on 64 x 64 masks made from the seed below, gated by each configuration's boxes as
the script gates them (`mask[y1:y2, x1:x2]`, sweep_bagls_conf.py:219-221).  Stored: the script, the boxes, the (Dice, IoU) lists.
The masks are NOT stored; tests/test_sweep_host.py regenerates them from `mask_seed` and `mask_density`.

The scripted confidences are drawn from a continuous distribution and none equals a threshold, so the fake's `>=` and the real
detector's `>` agree on every frame.
"""
from __future__ import annotations

import importlib.util
import json
import os

import numpy as np

import gen_golden as GG

HERE = os.path.dirname(os.path.abspath(__file__))

SHAPE = (64, 64)
N = 120
SCRIPT_SEED = 41
MASK_SEED = 20240
MASK_DENSITY = 0.3
CONFS = [0.1, 0.25, 0.5]
HOLDS = [0, 1, 3, 20, 999999]


def make_script():
    rs = np.random.RandomState(SCRIPT_SEED)
    H, W = SHAPE
    cx, cy = 30.0, 34.0
    script = []
    for _ in range(N):
        if rs.rand() < 0.25:
            script.append([])
            continue
        u = rs.rand()
        if u < 0.08:
            cx, cy = rs.uniform(12, W - 12), rs.uniform(12, H - 12)          # a far jump now and then
        cx = float(np.clip(cx + rs.uniform(-5, 5), 10, W - 10))
        cy = float(np.clip(cy + rs.uniform(-5, 5), 10, H - 10))
        w, h = rs.uniform(6, 28, 2)
        x1, y1, x2, y2 = max(0.0, cx - w / 2), max(0.0, cy - h / 2), min(float(W), cx + w / 2), min(float(H), cy + h / 2)
        script.append([[float(np.float32(v)) for v in (x1, y1, x2, y2, rs.uniform(0.02, 1.0))]])
    return script


def main() -> None:
    GG.install_placeholders()
    from openglottal.models.detector import TemporalDetector

    spec = importlib.util.spec_from_file_location("ref_sweep_bagls_conf", os.path.join(GG.REF, "scripts", "sweep_bagls_conf.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    H, W = SHAPE
    script = make_script()
    assert all(abs(d[0][4] - c) > 1e-6 for d in script if d for c in CONFS)
    rs = np.random.RandomState(MASK_SEED)
    pred = ((rs.rand(N, H, W) < MASK_DENSITY) * 255).astype(np.uint8)
    gt = ((rs.rand(N, H, W) < MASK_DENSITY) * 255).astype(np.uint8)
    frame = np.zeros((H, W, 3), np.uint8)
    out = {"shape": [H, W], "script": script, "mask_seed": MASK_SEED, "mask_density": MASK_DENSITY, "confs": CONFS, "holds": HOLDS,
           "unet_only": [list(ref.frame_metrics(pred[i], gt[i])) for i in range(N)], "columns": []}
    for conf in CONFS:
        for hold in HOLDS:
            GG.ScriptedYOLO.script = script
            det = TemporalDetector("fake.pt", conf=conf, max_hold_frames=hold)
            boxes, metrics = [], []
            for i in range(N):
                b = det.detect(frame)
                m = np.zeros_like(pred[i])
                if b is not None:
                    x1, y1, x2, y2 = b
                    m[y1:y2, x1:x2] = pred[i][y1:y2, x1:x2]
                boxes.append(None if b is None else [int(v) for v in b])
                metrics.append(list(ref.frame_metrics(m, gt[i])))
            out["columns"].append({"conf": conf, "hold": hold, "boxes": boxes, "metrics": metrics})
    kinds = [sum(b is None for b in c["boxes"]) for c in out["columns"]]
    print("frames without a box per column:", kinds)
    with open(os.path.join(HERE, "sweep_traces.json"), "w") as f:
        json.dump(out, f)
    print("wrote sweep_traces.json", os.path.getsize(os.path.join(HERE, "sweep_traces.json")), "bytes")


if __name__ == "__main__":
    main()
