"""Scripted `best` rows for the tracker tests (tests/test_track_host.py, tests/test_gpu_track.py): seeded random walks that are built
to visit every branch of `TemporalDetector.update` (openglottal_amd/detector.py), with the boxes and states the PYTHON state machine
gives for them, computed once per process.

A walk is a list of rows ``x1, y1, x2, y2, conf`` (conf = -1: no detection) clipped to the frame as the detector clips them, plus a
``resets`` byte per frame.  The generator follows the Python detector's own centre, so that it can aim at it: a jump of exactly
``max_shift_px`` (integer offsets on a half-pixel grid are exact in f32), the same jump moved by one or two ulps of a corner, a
3-4-5 jump, a far jump, runs of misses one longer than ``max_hold_frames``, boxes wider than the frame (the clamp's bounds cross and
the corner goes negative: Python's slice then counts from the far edge), boxes hugging a corner, and resets.
"""
import numpy as np

from openglottal_amd.detector import TemporalDetector
from openglottal_amd.utils import normalize_box

# (kw of TemporalDetector, (H, W), steps, seed): the defaults and three other parameter sets, four frame shapes
SEGMENTS = [
    ({}, (256, 256), 40000, 11),
    (dict(max_shift_px=12.5, padding=0, max_hold_frames=0), (100, 120), 25000, 12),
    (dict(max_shift_px=7, padding=20, max_hold_frames=5), (480, 640), 25000, 13),
    (dict(max_shift_px=30, padding=8, max_hold_frames=3), (33, 700), 15000, 14),
]


def _none_backend(frame, conf):
    return np.zeros((0, 4), np.float32), np.zeros(0, np.float32)


def step_python(det, row, W, H, reset=False):
    """One frame through the Python state machine, as features._detect_block drives it -> the normalised int box."""
    if reset:
        det.reset()
    b = det.update(row[None, :4], row[None, 4], W, H) if row[4] >= 0 else det.update(None, None, W, H)
    return normalize_box(b, W, H)


def state_words(det):
    if det._centre is None:
        return (0.0, 0.0, 0, 0, 0, 0)
    return (float(det._centre[0]), float(det._centre[1]), int(det._size[0]), int(det._size[1]), int(det._misses), 1)


def walk(kw, shape, n, seed):
    """-> dict(best [n,5] f32, resets [n] u8, boxes [n,4] i32, states [n,6] f64, tags: name -> count, W, H, kw)."""
    H, W = shape
    rs = np.random.RandomState(seed)
    det = TemporalDetector(_none_backend, **kw)
    ms = float(det.max_shift)
    best = np.zeros((n, 5), np.float32)
    resets = np.zeros(n, np.uint8)
    boxes = np.zeros((n, 4), np.int32)
    states = np.zeros((n, 6), np.float64)
    tags = {}
    pending_misses = 0
    for i in range(n):
        c = det._centre
        u = rs.rand()
        tag = "hit"
        hw, hh = rs.randint(2, 40), rs.randint(2, 40)          # half sizes of the raw box, whole pixels
        if pending_misses:
            pending_misses -= 1
            tag = "miss"
        elif c is None or u < 0.50:                              # a detection near the centre (or anywhere without one)
            if c is None:
                cx, cy = float(rs.randint(hw, W - hw + 1) if W > 2 * hw else W // 2), float(rs.randint(hh, H - hh + 1) if H > 2 * hh else H // 2)
            else:
                cx = float(np.round(c[0] * 2) / 2) + rs.randint(-6, 7) * 0.5
                cy = float(np.round(c[1] * 2) / 2) + rs.randint(-6, 7) * 0.5
                if rs.rand() < 0.02:
                    hw = 0                                       # no width: an empty slice where padding is 0
        elif u < 0.62:                                           # misses: now and then one more than the hold
            pending_misses = rs.choice([0, 0, 1, det.max_hold_frames, det.max_hold_frames + 1])
            tag = "miss"
        elif u < 0.80:                                           # a jump aimed at max_shift_px
            kind = rs.randint(4)
            if kind == 0:
                dx, dy = (ms, 0.0) if rs.rand() < 0.5 else (0.0, -ms)
            elif kind == 1:
                dx, dy = 0.6 * ms * rs.choice([-1, 1]), 0.8 * ms * rs.choice([-1, 1])
            elif kind == 2:
                a = rs.rand() * 2 * np.pi
                dx, dy = ms * np.cos(a), ms * np.sin(a)
            else:
                dx, dy = ms + rs.choice([-1, 1]) * rs.choice([0.5, 1.0]), 0.0
            cx, cy = float(c[0]) + dx, float(c[1]) + dy
            tag = "aimed"
        elif u < 0.86:                                           # far away: rejected
            cx, cy = float(c[0]) + rs.choice([-1, 1]) * (ms + 40 + rs.rand() * 50), float(c[1]) + rs.randn() * 5
            tag = "far"
        elif u < 0.93:                                           # wider / taller than the frame, or hugging a corner
            if rs.rand() < 0.5:
                hw, hh = W // 2 + rs.randint(0, 3), rs.choice([hh, H // 2 + rs.randint(0, 3)])
                cx, cy = W / 2.0, float(c[1]) if hh < H // 2 else H / 2.0
            else:
                cx, cy = rs.choice([0.0, 1.5, W - 1.0, float(W)]), rs.choice([0.0, 2.0, H - 0.5, float(H)])
            tag = "edge"
        else:
            resets[i] = 1
            cx, cy = float(rs.randint(0, W + 1)), float(rs.randint(0, H + 1))
            tag = "reset"
        if tag == "miss":
            row = np.array([0, 0, 0, 0, -1], np.float32)
        else:
            row = np.array([cx - hw, cy - hh, cx + hw, cy + hh, 0.3 + 0.6 * rs.rand()], np.float32)
            if tag == "aimed" and rs.rand() < 0.5:               # move one corner by an ulp or two: the centre moves by at most one
                k = rs.randint(4)
                for _ in range(rs.randint(1, 3)):
                    row[k] = np.nextafter(row[k], np.float32(rs.choice([-1e9, 1e9])))
            row[[0, 2]] = row[[0, 2]].clip(0, W)                 # the detector's own clip to the frame
            row[[1, 3]] = row[[1, 3]].clip(0, H)
        best[i] = row
        before = det._centre is not None
        boxes[i] = step_python(det, row, W, H, bool(resets[i]))
        states[i] = state_words(det)
        if row[4] < 0 and before and det._centre is None:
            tags["hold ran out"] = tags.get("hold ran out", 0) + 1
        if row[4] < 0 and det._centre is not None:
            tags["held"] = tags.get("held", 0) + 1
        if tuple(boxes[i]) == (0, 0, 0, 0):
            tags["empty slice"] = tags.get("empty slice", 0) + 1
        tags[tag] = tags.get(tag, 0) + 1
    # what the aimed jumps hit, from the recorded states (vectorised; the numbers only describe the walk)
    prev = np.vstack([np.zeros((1, 6)), states[:-1]])
    live = (best[:, 4] >= 0) & (prev[:, 5] == 1) & (resets == 0)
    j = np.hypot((best[:, 0] + best[:, 2]) / 2 - prev[:, 0].astype(np.float32), (best[:, 1] + best[:, 3]) / 2 - prev[:, 1].astype(np.float32))
    assert j.dtype == np.float32
    tags["jump == max_shift"] = int((live & (j == np.float32(ms))).sum())
    tags["jump within 4 ulp"] = int((live & (j != np.float32(ms)) & (np.abs(j.astype(np.float64) - ms) <= 4 * float(np.spacing(np.float32(ms))))).sum())
    tags["jump rejected"] = int((live & (j > np.float32(ms))).sum())
    has = states[:, 5] == 1
    tags["wider than the frame"] = int((has & ((states[:, 2] > W) | (states[:, 3] > H))).sum())
    hw2, hh2 = states[:, 2] // 2, states[:, 3] // 2
    tags["negative corner"] = int((has & ((np.minimum(np.maximum(states[:, 0], hw2), W - hw2).astype(np.int64) - hw2 < 0)
                                          | (np.minimum(np.maximum(states[:, 1], hh2), H - hh2).astype(np.int64) - hh2 < 0))).sum())
    return dict(best=best, resets=resets, boxes=boxes, states=states, tags=tags, W=W, H=H, kw=kw)


_CACHE = {}


def walks():
    """The four segments, computed once per process."""
    if "w" not in _CACHE:
        _CACHE["w"] = [walk(*s) for s in SEGMENTS]
    return _CACHE["w"]


def short_walk(n=700, seed=5, kw=None, shape=(256, 256)):
    key = ("s", n, seed, shape, tuple(sorted((kw or {}).items())))
    if key not in _CACHE:
        _CACHE[key] = walk(kw or {}, shape, n, seed)
    return _CACHE[key]


def trace_rows(script, conf):
    """A golden trace's script (lists of detections per frame) as `best` rows: the top-confidence detection at or above conf."""
    rows = np.zeros((len(script), 5), np.float32)
    for i, dets in enumerate(script):
        d = [x for x in dets if x[4] >= conf]
        if d:
            rows[i] = np.array(d, np.float32)[int(np.argmax(np.array([x[4] for x in d], np.float32)))]
        else:
            rows[i, 4] = -1
    return rows
