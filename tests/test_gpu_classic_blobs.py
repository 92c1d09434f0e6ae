"""-m gpu: k_blobs (raw mask, hole fill, labelling, keys, top-n, paint, count: one workgroup per frame) through
og_vft_guided_u8_dev against og_blobs_host, on the named masks of tests/classic_cases.py and on batches that cross a micro-batch
boundary.  beta = 1 keeps the threshold at 128 (1.0 * t + 0.0 * cur), the box covers the frame and the frame is 0 where the mask is
set and 255 elsewhere, so the raw mask of the kernel IS the given mask.  Equality everywhere; every shape runs twice.
The hard masks (spiral, serpentine, nested rings, more roots than lanes, diagonal-only chains), windows that differ from the frame,
a workspace that has seen another window and the timed worst-case ladder are additionally held against scipy.ndimage, with the mask
requested and without (the areas-only path counts inside the window)."""
import numpy as np
import pytest
import torch

import classic_cases as K
from openglottal_amd import classic as CL

pytestmark = pytest.mark.gpu

_ENG = {}


def engine(n):
    if n not in _ENG:
        e = CL.Classic(beta=1.0, percentile=30, n_components=n)
        e.thresh = 128.0
        _ENG[n] = e
    return _ENG[n]


def run_dev(masks, n, chunk=32):
    """masks [B,H,W] {0,1} -> (mask [B,H,W], area [B]) from the resident entry."""
    e = engine(n)
    e.set_chunk(chunk)
    B, H, W = masks.shape
    frames = torch.from_numpy(np.where(masks > 0, 0, 255).astype(np.uint8)).cuda()
    boxes = torch.tensor([[0, 0, W, H]] * B, dtype=torch.int32).cuda()
    out = torch.full((B, H, W), 7, dtype=torch.uint8, device="cuda")
    area = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    th = torch.zeros(B, dtype=torch.float64, device="cuda")
    e.guided_vft_dev(frames, B, H, W, 1, boxes, area, out, th)
    e.sync()
    assert (th.cpu().numpy() == 128.0).all()
    return out.cpu().numpy(), area.cpu().numpy()


_HOST = {}


def host(m, n):
    key = (m.tobytes(), m.shape, n)
    if key not in _HOST:
        _HOST[key] = CL.blobs_host(m, n)
    return _HOST[key]


@pytest.mark.parametrize("n", K.NS)
def test_named_masks_equal_the_host_twin(n):
    by_shape = {}
    for name, m in K.named_masks():
        by_shape.setdefault(m.shape, []).append((name, m))
    for shape, group in by_shape.items():
        batch = np.stack([m for _, m in group])
        got = run_dev(batch, n)
        again = run_dev(batch, n)
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), shape       # the same bits twice
        for i, (name, m) in enumerate(group):
            want_mask, want_area = host(m, n)
            assert got[1][i] == want_area and np.array_equal(got[0][i], want_mask), (name, n, int(got[1][i]), want_area)


@pytest.mark.parametrize("B,chunk", [(1, 32), (3, 2), (70, 32)])
def test_batches_across_a_micro_batch_boundary(B, chunk):
    rs = np.random.RandomState(100 + B)
    dens = rs.choice([0.3, 0.5, 0.6], B)
    masks = (rs.rand(B, 32, 48) < dens[:, None, None]).astype(np.uint8)
    got = run_dev(masks, 2, chunk)
    again = run_dev(masks, 2, chunk)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    for i in range(B):
        want_mask, want_area = host(masks[i], 2)
        assert got[1][i] == want_area and np.array_equal(got[0][i], want_mask), i


def fresh(n):
    e = CL.Classic(beta=1.0, percentile=30, n_components=n, chunk=32)
    e.thresh = 128.0
    return e


def launch(e, masks, boxes=None, bgr=False, want_mask=True):
    """One call of the resident entry on the handle ``e``: masks [B,H,W] {0,1}, boxes as a detector gives them (default: the
    frame) -> (mask [B,H,W] | None, area [B]).  The outputs are pre-filled, so every byte has to be written."""
    from openglottal_amd.utils import normalize_box

    B, H, W = masks.shape
    f = np.where(masks > 0, 0, 255).astype(np.uint8)
    if bgr:                                           # B = G = R: the gray of (v, v, v) is v for 0 and for 255
        f = np.ascontiguousarray(np.repeat(f[..., None], 3, axis=-1))
    frames = torch.from_numpy(f).cuda()
    rows = [normalize_box(b, W, H) for b in ([(0, 0, W, H)] * B if boxes is None else boxes)]
    bx = torch.tensor(rows, dtype=torch.int32).cuda()
    out = torch.full((B, H, W), 7, dtype=torch.uint8, device="cuda") if want_mask else None
    area = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    th = torch.zeros(B, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()                          # the handle's stream does not wait for torch's
    e.guided_vft_dev(frames, B, H, W, 3 if bgr else 1, bx, area, out, th)
    e.sync()
    assert (th.cpu().numpy() == 128.0).all()
    return (out.cpu().numpy() if want_mask else None), area.cpu().numpy()


def check(e, masks, boxes, n, label, bgr=False):
    """The launch with the mask and the areas-only launch, each twice with the same bits, against scipy on ``mask & roi`` (the
    independent statement) and against the host twin.  -> (mask, area)."""
    B, H, W = masks.shape
    got = launch(e, masks, boxes, bgr)
    again = launch(e, masks, boxes, bgr)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), label
    only = launch(e, masks, boxes, bgr, want_mask=False)
    only_again = launch(e, masks, boxes, bgr, want_mask=False)
    assert only[0] is None and np.array_equal(only[1], only_again[1]), label
    for i in range(B):
        roi = K.roi_of((0, 0, W, H) if boxes is None else boxes[i], H, W)
        raw = masks[i] * roi
        s_mask, s_area = K.scipy_blobs_cached(raw, n)
        h_mask, h_area = host(raw, n)
        assert got[1][i] == s_area == h_area and only[1][i] == s_area, (label, i, int(got[1][i]), int(only[1][i]), s_area, h_area)
        assert np.array_equal(got[0][i], s_mask) and np.array_equal(got[0][i], h_mask), (label, i)
        assert not got[0][i][~roi].any(), (label, i)
    return got


@pytest.mark.parametrize("S", (33, 64, 96))
def test_hard_masks_one_batch_per_side(S):
    """Spiral, serpentine, nested rings, more roots than lanes (S*S/4 specks at 96), diagonal-only chains, ... in ONE launch, gray at
    n = 1, 2, 8 and once through k_blobs<3>."""
    names, masks = zip(*K.hard_masks(S))
    batch = np.stack(masks)
    for n in (1, 2, 8):
        check(fresh(n), batch, None, n, (S, n, names))
    check(fresh(2), batch, None, 2, (S, "bgr", names), bgr=True)
    if S == 96:
        assert int(dict(K.hard_masks(S))["specks"].sum()) > 1024        # more roots than the workgroup has lanes


def window_batch(m):
    """One window case under every box: [15,40,56]."""
    return np.stack([m] * len(K.WINDOW_BOXES))


def test_windows_of_many_sizes_in_one_launch():
    """The window is the ROI grown by one pixel and cut to the frame; label indices are window-local while a frame's label arrays
    stride by H*W.  Every 33 x 33 hard mask inside a 40 x 56 frame, bright and dark outside the square, all fifteen boxes of a mask
    in one launch."""
    boxes = list(K.WINDOW_BOXES)
    e = {n: fresh(n) for n in (1, 2, 8)}
    for name, m in K.window_cases():
        for n in e:
            check(e[n], window_batch(m), boxes, n, (name, n), bgr=(n == 8))


def test_a_workspace_that_has_seen_another_window():
    """On ONE handle: 96 x 96 frames, the 40 x 56 windows, 96 x 96 again, then frames that alternate between no box and the whole
    frame -- each equal to what a fresh handle gives (and, through ``check``, to the references)."""
    big = np.stack([m for _, m in K.hard_masks(96)])
    win = [(name, m) for name, m in K.window_cases() if name in ("spiral+dark", "rings-inv", "specks+dark", "stairs-T")]
    assert len(win) == 4
    boxes = list(K.WINDOW_BOXES)
    alt = np.stack([m for _, m in K.hard_masks(64)])
    alt_boxes = [None if i % 2 == 0 else (0, 0, 64, 64) for i in range(len(alt))]
    e = fresh(2)
    steps = [("big", big, None)] + [(name, window_batch(m), boxes) for name, m in win]
    steps += [("big again", big, None), ("alternating", alt, alt_boxes)]
    for label, batch, bx in steps:
        got = check(e, batch, bx, 2, label)
        want = launch(fresh(2), batch, bx)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), label
    assert not got[1][0::2].any() and got[1][1::2].all()                # the frames without a box: area 0; the others: something


def test_worst_case_ladder_smallest_first():
    """The worst case of the labelling (one-pixel chains through the whole frame: spiral, its transpose, serpentine; nested rings for
    the hole fill) timed rung by rung, S = 32, 64, 128, 256.  A rung is launched only when the time predicted for it from the rungs
    before -- the last time x max(4, the last growth) -- stays under 2 s: past that the test FAILS without launching, so that a size
    nobody has measured never runs blind.  The 2 s is the condition for running at all, not a measurement.  B = 1, gray, box =
    frame, n = 2, mask requested; wall clock around sync(): one warm call, the median of three; a rung's time is its slowest mask."""
    import time

    e = fresh(2)
    times = []
    for S in K.LADDER_SIDES:
        if times:
            predicted = K.ladder_prediction(times)
            if predicted > K.LADDER_LIMIT_S:
                pytest.fail(f"side {S} not launched: {predicted:.3f} s predicted from {[round(t, 6) for t in times]} s")
        rung = []
        for name, m in K.ladder_masks(S):
            frames = torch.from_numpy(np.where(m > 0, 0, 255).astype(np.uint8)[None]).cuda()
            bx = torch.tensor([[0, 0, S, S]], dtype=torch.int32).cuda()
            out = torch.full((1, S, S), 7, dtype=torch.uint8, device="cuda")
            area = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            took = []
            for rep in range(4):
                out.fill_(7)
                area.fill_(-1)
                torch.cuda.synchronize()                                # the handle's stream does not wait for torch's
                t0 = time.perf_counter()
                e.guided_vft_dev(frames, 1, S, S, 1, bx, area, out, None)
                e.sync()
                took.append(time.perf_counter() - t0)
                s_mask, s_area = K.scipy_blobs_cached(m, 2)
                h_mask, h_area = host(m, 2)
                assert int(area.cpu()[0]) == s_area == h_area, (name, S, rep)
                got = out.cpu().numpy()[0]
                assert np.array_equal(got, s_mask) and np.array_equal(got, h_mask), (name, S, rep)
            rung.append(float(np.median(took[1:])))
            print(f"worst case {name} {S}x{S}: {rung[-1] * 1e3:.3f} ms (warm call {took[0] * 1e3:.3f} ms)")
        times.append(max(rung))
    print("worst case per side (ms): " + ", ".join(f"{S}: {t * 1e3:.3f}" for S, t in zip(K.LADDER_SIDES, times)))
    assert len(times) == len(K.LADDER_SIDES)


@pytest.mark.parametrize("B,H,W", [(8, 256, 256), (2, 120, 160)])
def test_larger_frames(B, H, W):
    """More pixels than one pass of the workgroup: smooth blobs with holes and specks, as a thresholded frame looks."""
    rs = np.random.RandomState(H)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for _ in range(4):
            cy, cx, ry, rx = rs.randint(20, H - 20), rs.randint(20, W - 20), rs.randint(5, 30), rs.randint(5, 40)
            d = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
            masks[b][(d < 1) & (d > 0.2 * (b % 3))] = 1
        masks[b][rs.rand(H, W) < 0.01] ^= 1
    got = run_dev(masks, 2)
    again = run_dev(masks, 2)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    for b in range(B):
        want_mask, want_area = host(masks[b], 2)
        assert got[1][b] == want_area and np.array_equal(got[0][b], want_mask), b
    assert got[1].min() > 0
