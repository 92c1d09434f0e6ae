"""The rules of the training-free family (include/openglottal_hip_classic.h) through their host twins, which run the very inline
functions the kernels call: the percentile against np.percentile, the threshold recurrence against Python floats, Otsu against a
float64 numpy statement, the blob filter against scipy.ndimage.  Every comparison is equality, bit for bit.  No GPU."""
import struct

import numpy as np
import pytest

import classic_cases as K
from openglottal_amd import classic as CL


def bits(x):
    return struct.pack("<d", float(x))


def hist_of(a):
    return np.bincount(np.asarray(a, np.uint8).ravel(), minlength=256).astype(np.uint32)


def test_percentile_equals_numpy_bit_for_bit():
    rs = np.random.RandomState(1234)
    qs = (0, 5, 30, 50, 100)
    cases = [np.array([7], np.uint8), np.array([3, 250], np.uint8), np.arange(11, dtype=np.uint8) * 20, np.full(57, 99, np.uint8),
             np.full(1, 0, np.uint8), np.full(2, 255, np.uint8)]
    sizes = [1, 2, 11, 12, 97, 1000, 5000]
    while len(cases) < 5000:                # 5 000 seeded arrays, every third of a listed size (a third of those n >= 1000)
        n = sizes[len(cases) % len(sizes)] if len(cases) % 3 == 0 else int(rs.randint(1, 600))
        lo = int(rs.randint(0, 200))
        hi = int(rs.randint(lo + 1, 257))
        cases.append(rs.randint(lo, hi, n).astype(np.uint8))
    checked = 0
    for a in cases:
        h = hist_of(a)
        for q in qs:
            want = float(np.percentile(a, q))
            got = CL.percentile_host(h, q)
            assert bits(got) == bits(want), (a.size, q, got, want)
            checked += 1
    assert len(cases) == 5000 and checked == 25000


def test_percentile_refuses_an_empty_histogram_and_a_bad_q():
    from openglottal_amd._lib import OpenGlottalHipError

    with pytest.raises(OpenGlottalHipError, match="empty histogram"):
        CL.percentile_host(np.zeros(256, np.uint32), 30)
    with pytest.raises(OpenGlottalHipError):
        CL.percentile_host(hist_of([1, 2, 3]), 101)


def test_recurrence_equals_python_floats_over_500_steps():
    rs = np.random.RandomState(9)
    for beta, q in ((0.7, 30), (0.9, 5), (0.35, 50)):
        t_ref = float(np.percentile(rs.randint(0, 256, 400).astype(np.uint8), q))
        t = t_ref
        small = 0
        for step in range(500):
            n = int(rs.randint(0, 11)) if step % 7 in (2, 3) else int(rs.randint(11, 900))     # n <= 10: the threshold is its own input
            px = rs.randint(0, 256, n).astype(np.uint8)
            cur = float(np.percentile(px, q)) if px.size > 10 else t_ref
            t_ref = beta * t_ref + (1 - beta) * cur
            t, cut = CL.vft_step_host(t, beta, hist_of(px), q)
            assert bits(t) == bits(t_ref), (beta, step, n)
            assert cut == min(256, max(0, int(np.ceil(t_ref))))
            small += n <= 10
        assert small > 100


def test_a_frame_without_pixels_still_moves_the_threshold():
    """0.7 t + 0.3 t is not always t: the recurrence is not skipped for a frame without a box."""
    empty = np.zeros(256, np.uint32)
    moved = 0
    for t0 in np.random.RandomState(3).rand(200) * 255:
        t, _ = CL.vft_step_host(float(t0), 0.7, empty, 30)
        assert bits(t) == bits(0.7 * float(t0) + (1 - 0.7) * float(t0))
        moved += t != float(t0)
    assert moved > 0


def test_cut_is_the_ceiling_clamped():
    empty = np.zeros(256, np.uint32)
    for t0, want in ((0.0, 0), (-3.5, 0), (0.25, 1), (12.0, 12), (12.000001, 13), (255.5, 256), (300.0, 256), (1e300, 256)):
        t, cut = CL.vft_step_host(t0, 1.0, empty, 30)      # beta 1: 1.0 * t + 0.0 * t = t
        assert t == t0 and cut == want, (t0, cut)


def test_otsu_equals_the_numpy_statement():
    rs = np.random.RandomState(5)
    cases = {
        "bimodal": np.concatenate([rs.normal(60, 10, 900), rs.normal(180, 15, 600)]).clip(0, 255).astype(np.uint8),
        "constant": np.full(300, 77, np.uint8),
        "two-valued": np.array([10] * 40 + [200] * 25, np.uint8),
        "single-pixel": np.array([131], np.uint8),
        "zeros": np.zeros(50, np.uint8),
        "skewed": np.array([0] * 100000 + [255], np.uint8),
    }
    for k in range(40):
        cases[f"random-{k}"] = rs.randint(int(rs.randint(0, 100)), int(rs.randint(101, 257)), int(rs.randint(1, 3000))).astype(np.uint8)
    for name, a in cases.items():
        h = hist_of(a)
        assert CL.otsu_threshold_host(h) == K.otsu_numpy(h), name
    assert CL.otsu_threshold_host(hist_of(cases["constant"])) == 0          # nothing qualifies
    assert CL.otsu_threshold_host(hist_of(cases["two-valued"])) == 10
    assert 60 < CL.otsu_threshold_host(hist_of(cases["bimodal"])) < 180


def test_box_hist_follows_python_slices_for_gray_and_bgr():
    from openglottal_amd.utils import bgr_to_gray_numpy

    rs = np.random.RandomState(8)
    bgr = rs.randint(0, 256, (32, 48, 3), dtype=np.uint8)
    gray = bgr_to_gray_numpy(bgr)
    for box in (None, (3, 4, 20, 30), (-10, -5, 40, 31), (40, 20, 90, 70), (10, 10, 10, 25), (30, 5, 12, 25), (0, 0, 48, 32), (-8, 0, -1, 32)):
        want = np.zeros(256, np.uint32) if box is None else hist_of(gray[box[1]:box[3], box[0]:box[2]])
        assert np.array_equal(CL.box_hist_host(gray, box), want), box
        assert np.array_equal(CL.box_hist_host(bgr, box), want), box


@pytest.mark.parametrize("n", K.NS)
def test_blob_filter_equals_scipy_on_the_named_masks(n):
    for name, m in K.named_masks():
        want_mask, want_area = K.scipy_blobs(m, n)
        got_mask, got_area = CL.blobs_host(m, n)
        assert got_area == want_area and np.array_equal(got_mask, want_mask), (name, n, got_area, want_area)
        assert CL.blobs_host(m * 255, n, want_mask=False) == (None, want_area)


def test_what_the_named_masks_are_there_for():
    masks = dict(K.named_masks())
    ring, area = CL.blobs_host(masks["ring"], 1)
    assert area == 49 and ring[5, 6] == 255                          # the hole is filled
    assert CL.blobs_host(masks["ring+island"], 1)[1] == 49           # the island belongs to the ring
    d, area = CL.blobs_host(masks["diamond"], 1)
    assert d[4, 4] == 255 and area == 25                             # closed by diagonal steps only: a hole
    assert CL.blobs_host(masks["corner-touch"], 1)[1] == 9 + 16      # one 8-connected blob
    comb = masks["comb"]
    assert CL.blobs_host(comb, 1)[1] == int(comb.sum())              # open pockets are not holes
    assert CL.blobs_host(masks["spiral"], 1)[1] == int(masks["spiral"].sum())
    assert CL.blobs_host(masks["top-row"], 1)[1] == int(masks["top-row"].sum()) == 21
    # the spiral IS one: it turns (pixels below row 0), it is one 8-connected chain, its channel is one 4-connected background open
    # to the border (no hole), and it has the pixel count of a spiral at every side the tests use
    from scipy import ndimage

    for S, count in ((21, 241), (64, 2112), (128, 8320), (256, 33024)):
        sp = K.spiral(S)
        assert int(sp.sum()) == count and int(sp[1:].sum()) == count - S, S
        assert ndimage.label(sp, structure=np.ones((3, 3), int))[1] == 1, S
        assert ndimage.label(sp == 0)[1] == 1 and sp[1, 0] == 0, S
        assert dict(K.hard_masks(S))["spiral"].tobytes() == sp.tobytes()
    assert np.array_equal(masks["spiral"], K.spiral(21)) and int(masks["spiral"][1:].sum()) == 220
    spk, area = CL.blobs_host(masks["specks+blob"], 2)
    assert area == 17 and spk[13, 15] == 255 and spk[0, 3] == 0      # key 0 ties: the speck that comes last in raster order
    tie, area = CL.blobs_host(masks["key-tie"], 1)
    assert area == 12 and tie[8, 13] == 255 and tie[2, 2] == 0       # equal keys: the later rectangle
    assert CL.blobs_host(masks["empty"], 2)[1] == 0 and CL.blobs_host(masks["full"], 2)[1] == 99


@pytest.mark.parametrize("S", (33, 64, 96, 128, 256))
def test_blob_filter_equals_scipy_on_the_hard_masks(S):
    """Spiral, serpentine, nested rings, S*S/4 specks of key 0, diagonal-only chains, checkerboard, comb; each also transposed,
    rotated and inverted."""
    masks = K.hard_masks(S)
    assert len(masks) == 28 and len({name for name, _ in masks}) == 28 and all(m.shape == (S, S) and m.max() <= 1 for _, m in masks)
    for name, m in masks:
        for n in K.NS:
            want_mask, want_area = K.scipy_blobs_cached(m, n)
            got_mask, got_area = CL.blobs_host(m, n)
            assert got_area == want_area and np.array_equal(got_mask, want_mask), (name, S, n, got_area, want_area)
            assert CL.blobs_host(m * 255, n, want_mask=False) == (None, want_area)
    by = dict(masks)
    half = (S + 1) // 2
    assert CL.blobs_host(by["rings"], 1)[1] == S * S                                  # a hole in a hole in a hole: all filled
    assert CL.blobs_host(by["spiral"], 8)[1] == int(by["spiral"].sum())               # one blob without a hole
    assert CL.blobs_host(by["serpentine"], 8)[1] == int(by["serpentine"].sum()) == half * S + (S - 1) // 2
    spk, area = CL.blobs_host(by["specks"], 8)                                        # half * half blobs of key 0: the last eight
    assert int(by["specks"].sum()) == half * half and area == 8
    assert np.array_equal(np.flatnonzero(spk), np.flatnonzero(by["specks"])[-8:])
    assert CL.blobs_host(by["stairs"], 1)[1] < int(by["stairs"].sum())                # separate diagonals, not one blob
    cb = by["checkerboard"]                                                           # one blob; every inner gap is a hole
    open_gaps = (cb[0] == 0).sum() + (cb[-1] == 0).sum() + (cb[1:-1, 0] == 0).sum() + (cb[1:-1, -1] == 0).sum()
    assert CL.blobs_host(cb, 1)[1] == S * S - int(open_gaps)                          # all but the gaps on the border
    assert CL.blobs_host(by["comb"], 1)[1] == int(by["comb"].sum())                   # open pockets


@pytest.mark.parametrize("S", (33, 64))
def test_blob_filter_equals_the_contour_statement_on_the_hard_masks(S):
    """Three statements by three algorithms: union-find over 2x2 windows (the library), scipy's labelling, and border following +
    shoelace + polygon fill composed as the reference's ``_nblobs`` (tests/golden/gen_golden_vft.py)."""
    for name, m in K.hard_masks(S):
        for n in (1, 8):
            c_mask, c_area = K.contour_blobs(m, n)
            s_mask, s_area = K.scipy_blobs_cached(m, n)
            h_mask, h_area = CL.blobs_host(m, n)
            assert c_area == s_area == h_area, (name, S, n, c_area, s_area, h_area)
            assert np.array_equal(c_mask, s_mask) and np.array_equal(c_mask, h_mask), (name, S, n)


def test_window_cases_through_the_host_composition():
    """Every 33 x 33 hard mask inside a 40 x 56 frame, bright and dark outside the square, under boxes that touch zero, one and two
    frame edges, a column, a row, a pixel, negative coordinates and a box leaving the frame: ``guided_vft_host`` at beta 1 and
    threshold 128 (the cut stays at 128; the frame is 0 where the mask is set and 255 elsewhere) equals scipy on ``mask & roi``."""
    H, W = K.WINDOW_FRAME
    boxes = list(K.WINDOW_BOXES)
    rois = [K.roi_of(b, H, W) for b in boxes]
    assert len(boxes) == 15 and all(r.any() for r in rois)
    checked = 0
    for name, m in K.window_cases():
        frame = np.where(m > 0, 0, 255).astype(np.uint8)
        for n in (1, 2, 8):
            masks, areas, ths, last = CL.guided_vft_host([frame] * len(boxes), boxes, 128.0, beta=1.0, n_components=n)
            assert last == 128.0 and (ths == 128.0).all()
            for i, roi in enumerate(rois):
                want_mask, want_area = K.scipy_blobs_cached(m * roi, n)
                assert areas[i] == want_area and np.array_equal(masks[i], want_mask), (name, n, boxes[i], int(areas[i]), want_area)
                assert not masks[i][~roi].any()
                checked += 1
    assert checked == 56 * 3 * 15


def test_blobs_host_refuses_bad_arguments():
    from openglottal_amd._lib import OpenGlottalHipError

    m = np.zeros((4, 4), np.uint8)
    for n in (0, 9, -1):
        with pytest.raises(OpenGlottalHipError, match="n_components"):
            CL.blobs_host(m, n)


def test_host_composition_equals_a_numpy_loop_of_process_frame():
    """guided_vft_host (the composition the GPU tests compare against) against the reference's statements written out in numpy
    with scipy as the blob filter."""
    rs = np.random.RandomState(21)
    H, W = 32, 48
    frames = rs.randint(0, 256, (12, H, W), dtype=np.uint8)
    frames[:, 8:20, 10:30] //= 3
    boxes = [(5, 4, 40, 28), None, None, (-3, -2, 30, 20), (44, 28, 60, 40), (10, 10, 10, 20), (6, 6, 9, 9), (0, 0, W, H)] * 2
    boxes = boxes[:12]
    t = float(np.percentile(frames[0][4:28, 5:40], 30))
    masks, areas, ths, last = CL.guided_vft_host(frames, boxes, t)
    tr = t
    for i, (f, b) in enumerate(zip(frames, boxes)):
        roi = np.zeros((H, W), bool)
        if b is not None:
            roi[b[1]:b[3], b[0]:b[2]] = True
        px = f[roi]
        cur = float(np.percentile(px, 30)) if px.size > 10 else tr
        tr = 0.7 * tr + (1 - 0.7) * cur
        raw = ((f < tr) & roi).astype(np.uint8)
        want, want_area = K.scipy_blobs(raw, 2)
        assert bits(ths[i]) == bits(tr) and areas[i] == want_area and np.array_equal(masks[i], want), i
    assert last == tr


def test_golden_sequences_through_the_host_twins():
    """The reference's own YOLOGuidedVFT (tests/golden/gen_golden_vft.py: contours by border following, shoelace and polygon fill)
    against the host twins composed in Python: seed, thresholds, areas and masks, gray and BGR."""
    from openglottal_amd.utils import bgr_to_gray_numpy

    for name, g in K.golden().items():
        frames, boxes, init = g["frames"], g["boxes"], g["init"]
        first = next((b for b in boxes[:init] if b is not None), None)
        h = CL.box_hist_host(frames[init - 1], first)
        if not h.any():
            h = CL.box_hist_host(frames[init - 1], (0, 0, frames.shape[2], frames.shape[1]))
        seed = CL.percentile_host(h, 30)
        assert bits(seed) == bits(g["seed"]), name
        for src in (frames[init:], bgr_to_gray_numpy(frames[init:])):
            masks, areas, ths, _ = CL.guided_vft_host(src, boxes[init:], seed)
            assert np.array_equal(ths.view(np.uint64), g["thresh"].view(np.uint64)), name
            assert np.array_equal(areas, g["area"]), name
            assert np.array_equal(np.stack(masks), g["masks"]), name
        assert any(b is None for b in boxes[init:]) and (g["area"] > 0).any()


def test_guided_vft_waveform_refuses_a_bad_init_count_before_touching_the_detector():
    from openglottal_amd import features as F

    class Untouched:
        model = None

        def reset(self):
            raise AssertionError("reset before the argument check")

    with pytest.raises(ValueError, match="ygvft_init"):
        F.guided_vft_area_waveform(np.zeros((4, 8, 8), np.uint8), Untouched(), ygvft_init=0)


def test_evaluate_refuses_classical_rows_without_a_detector():
    from openglottal_amd import evaluate as E

    with pytest.raises(ValueError, match="needs a detector"):
        E.evaluate(np.zeros((1, 8, 8), np.uint8), np.zeros((1, 8, 8), np.uint8), None, detector=None, classical=True)
