"""-m gpu: the sweep on the device (include/openglottal_hip_sweep.h: k_sweep_sat_rows, k_sweep_sat_cols, k_sweep_track, k_sweep_lookup)
against its host twin `og_sweep_host` -- the same inline functions, direct counting instead of tables -- so `frame_counts`,
`counts`, `boxes` and the final state of every configuration must be EQUAL.  The twin itself is held to the Python state machine,
to the tracker entry and to the reference's traces in tests/test_sweep_host.py."""
import numpy as np
import pytest
import torch

import sweep_cases as S
import track_cases as T
from openglottal_amd import gated, sweep

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_SW = {}


def handle():
    if "h" not in _SW:
        _SW["h"] = sweep.Sweep()
    return _SW["h"]


def grid(n_conf, n_hold, best):
    """Thresholds across the walk's confidences, one of them EQUAL to a confidence that occurs; holds 0.. and forever."""
    thr = np.linspace(0.3, 0.9, n_conf).tolist() if n_conf > 1 else [0.45]
    conf = best[best[:, 4] >= 0, 4]
    thr[n_conf // 2] = float(conf[len(conf) // 2])
    holds = list(range(n_hold - 1)) + [S.FOREVER]
    return thr, holds


def case(shape, n, seed=31):
    w = T.short_walk(n, seed, None, shape)
    pred, gt = S.masks_for(shape, n, 0.5)
    return w["best"], w["resets"], pred, gt


def up(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_dev(sw, pred, gt, best, resets, thr, holds, inclusive, want_boxes=True, **kw):
    n, H, W = pred.shape
    Cn = len(thr) * len(holds)
    d = [up(pred), up(gt), up(best), up(resets)]
    fc = torch.full((n, 3), -7, dtype=torch.int32, device=DEV)
    cnt = torch.full((Cn, n, 3), -7, dtype=torch.int32, device=DEV)
    box = torch.full((Cn, n, 4), -7, dtype=torch.int32, device=DEV) if want_boxes else None
    torch.cuda.synchronize()
    sw.counts_dev(d[0], d[1], d[2], n, H, W, thr, holds, fc, cnt, boxes_dev=box, resets_dev=d[3], inclusive=inclusive, **kw)
    sw.sync()
    return dict(frame_counts=fc.cpu().numpy(), counts=cnt.cpu().numpy(), boxes=None if box is None else box.cpu().numpy())


def same(got, want, keys=("frame_counts", "counts", "boxes")):
    for k in keys:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:5])


def states_equal(sw, states):
    for c in range(len(states)):
        assert sw.get_state(c).as_tuple() == states[c].as_tuple(), c


# (n_conf, n_hold, resets, inclusive): 1 configuration, 253 (a partial workgroup), 300 (two workgroups); both gates, with and without
GRIDS = [(1, 1, True, False), (11, 23, False, True), (10, 30, True, True), (11, 23, True, False)]


@pytest.mark.parametrize("shape,n", [((1, 1), 160), ((7, 13), 160), ((33, 257), 160), ((64, 64), 160), ((256, 256), 300)])
def test_the_device_equals_the_host_twin(shape, n):
    best, resets, pred, gt = case(shape, n)
    sw = handle()
    for n_conf, n_hold, with_resets, inclusive in GRIDS:
        thr, holds = grid(n_conf, n_hold, best)
        r = resets if with_resets else None
        states = (gated.TrackState * (n_conf * n_hold))()
        want = sweep.sweep_host(pred, gt, best, thr, holds, resets=r, inclusive=inclusive, states=states)
        assert want["counts"][:, :, 2].any() and not want["counts"][:, :, 2].all()
        sw.reset()
        got = run_dev(sw, pred, gt, best, r, thr, holds, inclusive)
        same(got, want)
        states_equal(sw, states)
        # the host-buffer entry: the same through the staging of micro-batches
        sw.reset()
        same(sw.counts(pred, gt, best, thr, holds, resets=r, inclusive=inclusive), want)
        states_equal(sw, states)
    # without the optional boxes the counts are the same
    sw.reset()
    same(run_dev(sw, pred, gt, best, r, thr, holds, inclusive, want_boxes=False), want, ("frame_counts", "counts"))
    # other scalars: they are read by every call, and changing them alone does not reset the states
    want2 = sweep.sweep_host(pred, gt, best, thr, holds, resets=r, inclusive=inclusive, max_shift_px=12.5, padding=0, states=states)
    same(run_dev(sw, pred, gt, best, r, thr, holds, inclusive, max_shift_px=12.5, padding=0), want2)
    states_equal(sw, states)


def test_results_do_not_depend_on_the_chunk_and_the_states_continue():
    shape, n = (40, 56), 300
    best, resets, pred, gt = case(shape, n, seed=32)
    thr, holds = [0.35, 0.5, 0.8], [0, 2, 7, S.FOREVER]
    states = (gated.TrackState * 12)()
    want = sweep.sweep_host(pred, gt, best, thr, holds, resets=resets, states=states)
    sw = sweep.Sweep()
    try:
        for chunk in (1, 64, 100, 0):
            sw.set_chunk(chunk)
            sw.reset()
            same(run_dev(sw, pred, gt, best, resets, thr, holds, False), want)
            states_equal(sw, states)
            sw.reset()
            same(sw.counts(pred, gt, best, thr, holds, resets=resets), want)
        # three calls of 100 frames equal one of 300: the states go from call to call
        sw.set_chunk(64)
        sw.reset()
        parts = [run_dev(sw, pred[a:a + 100], gt[a:a + 100], best[a:a + 100], resets[a:a + 100], thr, holds, False) for a in (0, 100, 200)]
        same({k: np.concatenate([p[k] for p in parts], 0 if k == "frame_counts" else 1) for k in parts[0]}, want)
        states_equal(sw, states)
        # without a reset the next call goes on from those states; another grid starts afresh
        st2 = (gated.TrackState * 12)(*states)
        cont = sweep.sweep_host(pred[:50], gt[:50], best[:50], thr, holds, states=st2)
        same(run_dev(sw, pred[:50], gt[:50], best[:50], None, thr, holds, False), cont)
        thr2 = [0.35, 0.5, 0.81]
        fresh = sweep.sweep_host(pred[:50], gt[:50], best[:50], thr2, holds)
        same(run_dev(sw, pred[:50], gt[:50], best[:50], None, thr2, holds, False), fresh)
    finally:
        sw.close()


def test_one_handle_across_shapes():
    """(40,56), then (33,257), then (40,56): the table's zero border lies elsewhere for another shape, so the third result equals the
    first only if every call rewrites it."""
    sw = sweep.Sweep()
    try:
        thr, holds = [0.4, 0.6], [0, 3, S.FOREVER]
        outs = []
        for shape in ((40, 56), (33, 257), (40, 56), (1, 1), (40, 56)):
            best, resets, pred, gt = case(shape, 120, seed=33)
            pred = np.full_like(pred, 255)                       # every table entry is nonzero where it may be
            sw.reset()
            got = run_dev(sw, pred, gt, best, resets, thr, holds, False)
            same(got, sweep.sweep_host(pred, gt, best, thr, holds, resets=resets))
            outs.append(got)
        same(outs[2], outs[0])
        same(outs[4], outs[0])
    finally:
        sw.close()


def test_single_pixels_at_the_corners_and_boxes_on_their_edges():
    """Exclusive tables: entry (y, x) counts rows < y and columns < x.  With padding 0, a reset before every frame and even sizes
    the tracker's box is the detection's own rectangle, so each expected count can be written down."""
    H, W = 8, 10
    rects = [((0, 0, 10, 8), 4), ((1, 1, 9, 7), 0), ((0, 0, 2, 2), 1), ((8, 6, 10, 8), 1), ((0, 6, 2, 8), 1), ((8, 0, 10, 2), 1),
             ((0, 0, 10, 2), 2), ((0, 1, 10, 7), 0), ((1, 0, 9, 8), 0), ((0, 0, 2, 8), 2), ((8, 0, 10, 8), 2), ((2, 2, 8, 6), 0)]
    n = len(rects)
    pred = np.zeros((n, H, W), np.uint8)
    pred[:, [0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = 9
    gt = pred.copy()
    gt[:, 0, 0] = 0                                             # the top-left corner is predicted but not true
    best = np.array([[*r, 0.9] for r, _ in rects], np.float32)
    resets = np.ones(n, np.uint8)
    sw = handle()
    sw.reset()
    got = run_dev(sw, pred, gt, best, resets, [0.5], [0], False, padding=0)
    same(got, sweep.sweep_host(pred, gt, best, [0.5], [0], resets=resets, padding=0))
    assert got["boxes"][0].tolist() == [list(r) for r, _ in rects]
    assert got["counts"][0, :, 1].tolist() == [k for _, k in rects]
    top_left = [int(r[0] == 0 and r[1] == 0) for r, _ in rects]
    assert got["counts"][0, :, 0].tolist() == [k - t for (_, k), t in zip(rects, top_left)]
    assert got["frame_counts"].tolist() == [[3, 4, 3]] * n


def test_a_full_mask_counts_box_areas():
    shape, n = (256, 256), 60
    best, resets, _, gt = case(shape, n, seed=34)
    pred = np.full((n,) + shape, 255, np.uint8)
    thr, holds = [0.3, 0.6], [0, 3]
    sw = handle()
    sw.reset()
    got = run_dev(sw, pred, gt, best, resets, thr, holds, False)
    b = got["boxes"]
    assert (b[:, :, 0] >= 0).any() and (b[:, :, 0] < 0).any()
    assert np.array_equal(got["counts"][:, :, 1], np.where(b[:, :, 0] >= 0, (b[:, :, 2] - b[:, :, 0]) * (b[:, :, 3] - b[:, :, 1]), 0))
    assert (got["frame_counts"][:, 1] == 256 * 256).all()
    same(got, sweep.sweep_host(pred, gt, best, thr, holds, resets=resets))
