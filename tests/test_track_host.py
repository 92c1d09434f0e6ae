"""The tracker rule on the host (`og_track_host`, the inline function `k_track_boxes` calls) against the Python state machine it
restates (`TemporalDetector.update`) and against the reference's own recorded traces.  No GPU."""
import ctypes as C
import json
import os

import numpy as np

import track_cases as T
from openglottal_amd import gated
from openglottal_amd.detector import TemporalDetector


def _params(kw):
    d = TemporalDetector(T._none_backend, **kw)
    return gated.params_of(d.max_shift, d.padding, d.max_hold_frames)


def test_the_golden_traces_of_the_reference(golden_dir):
    traces = json.load(open(os.path.join(golden_dir, "detector_traces.json")))
    assert len(traces) >= 9
    for name, t in traces.items():
        H, W = t["shape"][:2]
        kw = dict(t["kw"])
        conf = kw.get("conf", 0.25)
        rows = T.trace_rows(t["script"], conf)
        st = gated.TrackState()
        boxes = gated.track_host(st, _params(kw), rows, W, H)
        want = np.array([[-1] * 4 if b is None else b for b in t["out"]], np.int32)
        # the traces hold the detector's raw boxes; none of them leaves the frame, so normalize_box is the identity on them
        assert np.array_equal(boxes, want), (name, boxes.tolist(), want.tolist())
        det = TemporalDetector(T._none_backend, **kw)          # ... and TemporalDetector.track is the same call
        assert np.array_equal(det.track(rows, W, H), want), name


def test_the_walks_visit_every_branch():
    tags = {}
    for w in T.walks():
        for k, v in w["tags"].items():
            tags[k] = tags.get(k, 0) + v
    print(tags)
    assert sum(len(w["best"]) for w in T.walks()) >= 100000
    for k in ("hit", "miss", "held", "hold ran out", "aimed", "jump == max_shift", "jump within 4 ulp", "jump rejected", "far", "edge",
              "wider than the frame", "negative corner", "empty slice", "reset"):
        assert tags.get(k, 0) >= 20, (k, tags)
    for w in T.walks():                                          # every segment aims exactly at its own max_shift_px
        assert w["tags"].get("jump == max_shift", 0) >= 5 and w["tags"].get("hold ran out", 0) >= 5, w["tags"]


def test_one_call_equals_update_step_for_step():
    for w in T.walks():
        st = gated.TrackState()
        boxes = gated.track_host(st, _params(w["kw"]), w["best"], w["W"], w["H"], w["resets"])
        bad = np.flatnonzero((boxes != w["boxes"]).any(1))
        assert bad.size == 0, (w["kw"], bad[:5], boxes[bad[:5]], w["boxes"][bad[:5]], w["best"][bad[:5]])
        assert st.as_tuple() == tuple(w["states"][-1]), (st.as_tuple(), w["states"][-1])


def test_the_state_after_every_step_equals_the_python_state():
    for w in T.walks():
        n = 6000
        st, p = gated.TrackState(), _params(w["kw"])
        for i in range(n):
            b = gated.track_host(st, p, w["best"][i:i + 1], w["W"], w["H"], w["resets"][i:i + 1])
            assert tuple(b[0]) == tuple(w["boxes"][i]) and st.as_tuple() == tuple(w["states"][i]), (w["kw"], i, b, st.as_tuple(), w["states"][i])


def test_a_call_split_into_several_equals_one_call():
    rs = np.random.RandomState(3)
    for w in T.walks():
        n = 20000
        p = _params(w["kw"])
        one = gated.TrackState()
        whole = gated.track_host(one, p, w["best"][:n], w["W"], w["H"], w["resets"][:n])
        cuts = np.unique(np.concatenate([[0, 1, 2, 257, n], rs.randint(0, n, 40)]))
        st, parts = gated.TrackState(), []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            parts.append(gated.track_host(st, p, w["best"][lo:hi], w["W"], w["H"], w["resets"][lo:hi]))
        assert np.array_equal(np.concatenate(parts), whole) and st.as_tuple() == one.as_tuple()
        # and through the Python object: TemporalDetector.track continues from and leaves the object's state
        det = TemporalDetector(T._none_backend, **w["kw"])
        got = np.concatenate([det.track(w["best"][lo:hi], w["W"], w["H"], w["resets"][lo:hi]) for lo, hi in ((0, 300), (300, 301), (301, 2000))])
        assert np.array_equal(got, w["boxes"][:2000]) and T.state_words(det) == tuple(w["states"][1999])
        nxt = T.step_python(det, w["best"][2000], w["W"], w["H"], bool(w["resets"][2000]))     # update() goes on from track()'s state
        assert tuple(nxt) == tuple(w["boxes"][2000])


def test_the_hypot_of_the_rule_equals_numpy_on_f32():
    """2 000 000 seeded pairs, most of them within 1e-5 of 30 and many exactly 30.0: the jump the rule computes,
    (float)sqrt((double)dx*dx + (double)dy*dy), has np.hypot's f32 bits and makes np.hypot's decision.  The rule is driven through
    og_track_host: a state with its centre at the origin, one row per pair whose centre is (dx, dy); the row is accepted exactly
    when hypot(dx, dy) <= max_shift_px."""
    rs = np.random.RandomState(7)
    n = 2000000
    ang = rs.rand(n) * 2 * np.pi
    r = np.float32(30.0) + (rs.randint(-5, 6, n) * np.spacing(np.float32(30.0))).astype(np.float32)
    dx = (r * np.cos(ang)).astype(np.float32)
    dy = (r * np.sin(ang)).astype(np.float32)
    k = n // 8                                                   # exact triples scaled to 30, and the axes
    dx[:k], dy[:k] = np.float32(18.0), np.float32(24.0)
    dx[k:2 * k], dy[k:2 * k] = np.float32(30.0), np.float32(0.0)
    dx[2 * k:2 * k + 1000] = np.nextafter(np.float32(30.0), np.float32(31.0))
    dy[2 * k:2 * k + 1000] = 0
    ref = np.hypot(dx, dy)
    assert ref.dtype == np.float32
    near, equal = int((np.abs(ref.astype(np.float64) - 30.0) <= 1e-5).sum()), int((ref == np.float32(30.0)).sum())
    print(f"within 1e-5 of 30: {near}, exactly 30.0: {equal}")
    assert near >= 1000000 and equal >= 100000
    mine = np.sqrt(dx.astype(np.float64) * dx.astype(np.float64) + dy.astype(np.float64) * dy.astype(np.float64)).astype(np.float32)
    assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32))            # the formula's value, in numpy
    # the rule's own decision on the same pairs: frames alternate between [a reset and a row that puts the centre at the origin]
    # and [a row whose centre is exactly (dx, dy): x1 = x2 = dx, y1 = y2 = dy].  With max_hold_frames = 0 a rejected jump clears
    # the centre (box -1) and an accepted one moves it (an empty box, (0,0,0,0)).  (The rule does not need rows inside the frame.)
    rows = np.zeros((2 * n, 5), np.float32)
    rows[:, 4] = 1.0
    rows[1::2, 0] = rows[1::2, 2] = dx
    rows[1::2, 1] = rows[1::2, 3] = dy
    resets = np.zeros(2 * n, np.uint8)
    resets[0::2] = 1
    st = gated.TrackState()
    boxes = gated.track_host(st, gated.params_of(30, 0, 0), rows, 4096, 4096, resets)
    want = ref > np.float32(30.0)
    got = boxes[1::2, 0] < 0
    assert (boxes[0::2] == 0).all() and np.array_equal(got, want), int((got != want).sum())
    assert 100000 < int(want.sum()) < n - 100000                 # both decisions occur


def test_bad_arguments_are_refused_before_anything_is_written():
    from openglottal_amd._lib import lib

    l = lib()
    raw = np.zeros(4096, np.uint8)
    base = raw.ctypes.data + (-raw.ctypes.data) % 8
    st, par, best, boxes = base, base + 64, base + 128, base + 1024
    C.memmove(par, C.addressof(gated.params_of()), 12)
    before = raw.copy()
    assert l.og_track_host(st, par, best, None, 4, 64, 64, boxes) == 0
    raw[:] = before
    for off in (1, 2):
        assert l.og_track_host(st + off, par, best, None, 4, 64, 64, boxes) == -1
        assert l.og_track_host(st, par + off, best, None, 4, 64, 64, boxes) == -1
        assert l.og_track_host(st, par, best + off, None, 4, 64, 64, boxes) == -1
        assert l.og_track_host(st, par, best, None, 4, 64, 64, boxes + off) == -1
    assert l.og_track_host(None, par, best, None, 4, 64, 64, boxes) == -1
    assert l.og_track_host(st, None, best, None, 4, 64, 64, boxes) == -1
    assert l.og_track_host(st, par, None, None, 4, 64, 64, boxes) == -1
    assert l.og_track_host(st, par, best, None, 4, 64, 64, None) == -1
    assert l.og_track_host(st, par, best, None, -1, 64, 64, boxes) == -1
    assert l.og_track_host(st, par, best, None, 4, 0, 64, boxes) == -1
    assert np.array_equal(raw, before)
    assert l.og_track_host(st, par, best, best, 4, 64, 64, boxes) == 0            # resets: u8, any address
