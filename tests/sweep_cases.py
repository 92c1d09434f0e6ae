"""Cases and an independent oracle for the sweep tests (tests/test_sweep_host.py, tests/test_gpu_sweep*.py).

The oracle is the PYTHON state machine, once per configuration: `TemporalDetector(_none_backend, max_hold_frames=h).update`, fed the
frame's row where the gate lets it through and `None` where not, then numpy slicing `pred[y1:y2, x1:x2]` with the box as Python
returns it (the slice does the normalisation) and counting.  Nothing of the library is called.

Rows come from `track_cases.short_walk` (confidences in [0.3, 0.9), jumps at exactly `max_shift`, boxes wider than the frame,
resets).  Four rows that follow a reset -- there the state machine has no centre, so the gate alone decides whether the frame has a
box -- get chosen confidences: two keep their own (the grid takes them as thresholds), one becomes exactly 0.5 and one
`np.float32(0.5000001)`.
"""
import numpy as np

import track_cases as T
from openglottal_amd.detector import TemporalDetector
from openglottal_amd.utils import normalize_box

FOREVER = 2147483647
HOLDS = [0, 1, 3, 20, FOREVER]
SHAPES = [(1, 1), (7, 13), (40, 56), (33, 257)]
DENSITIES = [0.0, 0.5, 1.0]
JUST_ABOVE_HALF = np.float32(0.5000001)

_CACHE = {}


def rows_for(shape, n=160, seed=21):
    """-> dict(best [n,5] f32, resets [n] u8, W, H, own: two frame indices whose own confidence is a threshold, half: the frame with
    conf 0.5, above: the frame with conf f32(0.5000001), thresholds: the five of the grid)."""
    key = ("rows", shape, n, seed)
    if key in _CACHE:
        return _CACHE[key]
    w = T.short_walk(n, seed, None, shape)
    best, resets = w["best"].copy(), w["resets"].copy()
    after_reset = [i for i in range(n) if resets[i] and best[i, 4] >= 0]
    assert len(after_reset) >= 4, (shape, len(after_reset))
    a, b, half, above = after_reset[:4]
    best[half, 4] = np.float32(0.5)
    best[above, 4] = JUST_ABOVE_HALF
    assert float(JUST_ABOVE_HALF) > 0.5 and best[a, 4] != best[b, 4]
    thresholds = [0.0, float(np.float32(best[a, 4])), 0.5, float(np.float32(best[b, 4])), 0.95]
    _CACHE[key] = dict(best=best, resets=resets, W=shape[1], H=shape[0], own=(a, b), half=half, above=above, thresholds=thresholds)
    return _CACHE[key]


def masks_for(shape, n, density, seed=3):
    """Seeded noise: pred and gt [n,H,W] u8 with values in {0, 1..255} at the density."""
    rs = np.random.RandomState(seed + int(density * 10) + shape[0] * 7 + shape[1])
    H, W = shape
    out = []
    for _ in range(2):
        on = rs.rand(n, H, W) < density
        out.append((on * rs.randint(1, 256, (n, H, W))).astype(np.uint8))
    return out[0], out[1]


def oracle_boxes(best, resets, W, H, thresholds, holds, inclusive, max_shift_px=30, padding=8):
    """-> (raw [C][n] Python boxes or None, boxes [C,n,4] int32 normalised) by the Python state machine."""
    n = len(best)
    raw, boxes = [], np.zeros((len(thresholds) * len(holds), n, 4), np.int32)
    for it, thr in enumerate(thresholds):
        for ih, hold in enumerate(holds):
            det = TemporalDetector(T._none_backend, max_shift_px=max_shift_px, padding=padding, max_hold_frames=hold)
            col = []
            for i in range(n):
                if resets is not None and resets[i]:
                    det.reset()
                conf = float(best[i, 4])                      # a Python float that holds an f32
                ok = best[i, 4] >= 0 and (conf >= thr if inclusive else conf > thr)
                b = det.update(best[i:i + 1, :4], best[i:i + 1, 4], W, H) if ok else det.update(None, None, W, H)
                col.append(b)
                boxes[it * len(holds) + ih, i] = normalize_box(b, W, H)
            raw.append(col)
    return raw, boxes


def oracle_counts(pred, gt, raw):
    """-> (frame_counts [n,3], counts [C,n,3]) by numpy slicing."""
    n = len(pred)
    p, g = pred > 0, gt > 0
    fc = np.stack([(p & g).reshape(n, -1).sum(1), p.reshape(n, -1).sum(1), g.reshape(n, -1).sum(1)], 1).astype(np.int32)
    counts = np.zeros((len(raw), n, 3), np.int32)
    for c, col in enumerate(raw):
        for i, b in enumerate(col):
            if b is None:
                continue
            x1, y1, x2, y2 = b
            counts[c, i] = ((p[i][y1:y2, x1:x2] & g[i][y1:y2, x1:x2]).sum(), p[i][y1:y2, x1:x2].sum(), 1)
    return fc, counts


def oracle(shape, density, inclusive, n=160):
    key = ("oracle", shape, density, inclusive, n)
    if key not in _CACHE:
        r = rows_for(shape, n)
        bkey = ("boxes", shape, inclusive, n)
        if bkey not in _CACHE:
            _CACHE[bkey] = oracle_boxes(r["best"], r["resets"], r["W"], r["H"], r["thresholds"], HOLDS, inclusive)
        raw, boxes = _CACHE[bkey]
        pred, gt = masks_for(shape, n, density)
        fc, counts = oracle_counts(pred, gt, raw)
        _CACHE[key] = dict(pred=pred, gt=gt, frame_counts=fc, counts=counts, boxes=boxes, **r)
    return _CACHE[key]
