"""-m gpu: the tiled blob filter (include/openglottal_hip_classic_tiled.h; k_tblob_* of csrc/og_kernels.hpp) against the
one-workgroup k_blobs, the host twin and scipy.ndimage.  Masks are driven through the resident guided-VFT entry as in
tests/test_gpu_classic_blobs.py (gray encodes the mask, beta = 1 keeps the threshold at 128); every case runs with the mask requested
and with areas only, twice with the same bits.  Shapes are named from the tile edge T = og_classic_tiled_limit(1): a single tile,
frames whose seams and four-tile corners the hand-built masks sit on, frames above the old 65 536-pixel limit in mode "auto", the
Python surface, buffer extents at 300 x 260, and the worst-case ladder climbed to the declared limit.

Measured by the ladder test on an MI355X (the slowest of the four masks per side, ms): 32: 0.088, 64: 0.104,
128: 0.120, 256: 0.173, 512: 0.338, 1024: 0.937, 2048: 3.273 -- so every rung was predicted far under LADDER_LIMIT_S and launched."""
import numpy as np
import pytest
import torch

import buffer_guard as G
import classic_cases as K
import test_gpu_classic_blobs as TB
from openglottal_amd import classic as CL
from openglottal_amd import features as F
from openglottal_amd._lib import check, lib
from openglottal_amd.utils import bgr_to_gray, normalize_box

pytestmark = pytest.mark.gpu

T = int(lib().og_classic_tiled_limit(1))
LIMIT = int(lib().og_classic_tiled_limit(0))
FRAMES = ((2 * T + 3, T + 5), (T + 1, 2 * T + 1))          # H, W: three by two tiles, two by three tiles


def fresh(n, tiled):
    e = CL.Classic(beta=1.0, percentile=30, n_components=n, chunk=32, tiled=tiled)
    e.thresh = 128.0
    return e


def check_tiled(masks, boxes, n, label, tiled="always", bgr=False, e=None):
    """TB.check (mask and areas only, each twice, against scipy and the host twin) on a tiled handle."""
    return TB.check(e or fresh(n, tiled), masks, boxes, n, label, bgr)


def on_canvas(m, H, W, at=(0, 0)):
    """m cut to an H x W canvas at ``at``."""
    out = np.zeros((H, W), np.uint8)
    y, x = at
    h, w = min(m.shape[0], H - y), min(m.shape[1], W - x)
    out[y:y + h, x:x + w] = m[:h, :w]
    return out


# ── a single tile ────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("n", K.NS)
def test_single_tile_equals_the_one_workgroup_filter(n):
    """Every hard mask at side 33 (one tile and a one-pixel second one) in one launch, and every window case under its fifteen boxes
    in one launch: "always" equals "off" bit for bit, and both the references."""
    names, masks = zip(*K.hard_masks(33))
    batch = np.stack(masks)
    e, off = fresh(n, "always"), fresh(n, "off")
    got = check_tiled(batch, None, n, ("hard 33", n), e=e)
    want = TB.launch(off, batch)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), names
    boxes = list(K.WINDOW_BOXES)
    for name, m in K.window_cases():
        got = check_tiled(TB.window_batch(m), boxes, n, (name, n), e=e, bgr=(n == 8))
        want = TB.launch(off, TB.window_batch(m), boxes)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (name, n)


# ── seams ────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("H,W", FRAMES + ((2 * T + 1, 2 * T + 1),))
def test_hard_masks_across_seams(H, W):
    """Spiral, serpentine, rings, checkerboard, diagonal chains (stairs), ... at side 2T + 1, each also transposed, rotated and
    inverted, cut to the frame; the square frame holds them whole (three by three tiles)."""
    names, masks = zip(*K.hard_masks(2 * T + 1))
    assert {"spiral", "spiral-T", "serpentine", "serpentine-T", "rings", "rings-T", "checkerboard", "checkerboard-T", "stairs",
            "stairs-T"} <= set(names)
    batch = np.stack([on_canvas(m, H, W) for m in masks])
    for n in (1, 2, 8):
        check_tiled(batch, None, n, (H, W, n, names))
    check_tiled(batch, None, 2, (H, W, "bgr", names), bgr=True)


def one(m, n, label, boxes=None):
    got = check_tiled(m[None], boxes, n, label)
    return got[0][0], int(got[1][0])


@pytest.mark.parametrize("H,W", FRAMES)
def test_one_blob_across_a_four_tile_corner(H, W):
    m = np.zeros((H, W), np.uint8)
    m[T - 1, T - 1] = m[T, T] = 1
    m[3, 3] = 1                                                     # a speck that n = 1 must leave out
    out, area = one(m, 1, ("corner diagonal", H, W))
    assert area == 2 and out[T - 1, T - 1] and out[T, T] and not out[3, 3], "the diagonal across a four-tile corner is one blob"
    m = np.zeros((H, W), np.uint8)
    m[T - 1, T] = m[T, T - 1] = 1
    m[3, 3] = 1
    out, area = one(m, 1, ("corner anti-diagonal", H, W))
    assert area == 2 and out[T - 1, T] and out[T, T - 1] and not out[3, 3], "the anti-diagonal across a four-tile corner is one blob"


@pytest.mark.parametrize("H,W", FRAMES)
def test_a_hole_that_spans_a_seam_is_filled(H, W):
    m = np.zeros((H, W), np.uint8)
    y, x = min(T - 5, H - 11), min(T - 6, W - 11)                   # an 11 x 11 one-pixel ring that fits the frame
    m[y:y + 11, x:x + 11] = 1
    m[y + 1:y + 10, x + 1:x + 10] = 0
    assert x + 1 < T < x + 9 and (H < 2 * T or y + 1 < T < y + 9)   # its hole lies on both sides of a seam (four tiles in the tall frame)
    out, area = one(m, 1, ("ring across a seam", H, W))
    assert area == 11 * 11 and out[y:y + 11, x:x + 11].all(), "the hole across the seams is filled"


@pytest.mark.parametrize("H,W", FRAMES)
def test_a_pocket_open_through_the_next_tile_is_not_filled(H, W):
    tr = H < 2 * T                                                  # the wide frame: the same mask transposed, across the vertical seam
    m = np.zeros((W, H) if tr else (H, W), np.uint8)
    m[T - 6:T + 7, 3:13] = 1
    m[T - 5:T + 6, 4:12] = 0                                        # a ring over the seam between tile rows 0 and 1 ...
    m[T - 6, 7] = 0                                                 # ... open at the top, in the upper tile
    ring = int(m.sum())
    assert m[T + 6, 3:13].all()                                     # (it fits: the bottom wall is there)
    out, area = one(np.ascontiguousarray(m.T) if tr else m, 1, ("open pocket", H, W))
    out = out.T if tr else out
    assert area == ring and not out[T:T + 6, 4:12].any(), "the pocket reaches the border through the next tile: not a hole"


@pytest.mark.parametrize("H,W", FRAMES)
def test_specks_in_four_tiles_tie_to_the_later_pixel(H, W):
    m = np.zeros((H, W), np.uint8)
    at = [(2, 2), (5, T + 2), (T, 1), (T, T + 3)]                     # one per tile, raster order
    for y, x in at:
        m[y, x] = 1
    out, area = one(m, 2, ("specks", H, W))
    assert area == 2 and out[at[2]] and out[at[3]] and not out[at[0]] and not out[at[1]], "equal keys: the later first pixel wins"


def test_eight_blobs_in_eight_tiles():
    """Blocks of 2 x k pixels, k = 1..8 (keys 2 (k - 1): all distinct), one per tile.  Eight tiles need more than the six of the two
    seam frames: (2T + 3) x (2T + 11), three by three tiles with a 3-pixel last row and an 11-pixel last column of tiles."""
    H, W = 2 * T + 3, 2 * T + 11
    m = np.zeros((H, W), np.uint8)
    tiles = [(r, c) for r in range(3) for c in range(3)][:8]
    order = [5, 2, 8, 1, 7, 3, 6, 4]                                  # sizes not in raster order
    for (r, c), k in zip(tiles, order):
        y = r * T + 1 if r < 2 else 2 * T + 1
        m[y:y + 2, c * T + 1:c * T + 1 + k] = 1
    out, area = one(m, 8, "eight blobs n=8")
    assert area == 2 * 36 and np.array_equal(out > 0, m > 0)
    out, area = one(m, 3, "eight blobs n=3")
    assert area == 2 * (8 + 7 + 6)
    for (r, c), k in zip(tiles, order):
        y = r * T + 1 if r < 2 else 2 * T + 1
        assert bool(out[y, c * T + 1]) == (k >= 6), (r, c, k)


@pytest.mark.parametrize("H,W", FRAMES)
def test_windows_that_start_mid_tile_leave_the_frame_or_are_missing(H, W):
    rs = np.random.RandomState(H)
    names, masks = zip(*[(k, v) for k, v in K.hard_masks(2 * T + 1) if k in ("spiral", "rings", "serpentine-T", "stairs", "checkerboard-inv")])
    batch = np.stack([on_canvas(m, H, W) for m in masks] + [(rs.rand(H, W) < d).astype(np.uint8) for d in (0.3, 0.5, 0.6)])
    B = len(batch)
    mid = (T - 2, T - 3, 2 * T + 2, T + 4)
    assert mid[0] % T and mid[1] % T                                 # starts inside a tile
    check_tiled(batch, [mid] * B, 2, ("window mid-tile", H, W))
    check_tiled(batch, [(T - 1, T - 3, W + 40, H + 9)] * B, 2, ("box leaving the frame", H, W))
    check_tiled(batch, [(-W + 2, -H + 1, -1, -2)] * B, 8, ("box from the far edge", H, W))
    alt = [None if i % 2 == 0 else (0, 0, W, H) for i in range(B)]
    got = check_tiled(batch, alt, 2, ("alternating with None", H, W))
    assert not got[1][0::2].any() and got[1][1::2].all() and not got[0][0::2].any()


# ── above the old limit, "auto" ─────────────────────────────────────────────────
def blobby(B, H, W, seed):
    """Smooth blobs with holes and specks, as a thresholded frame looks."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for _ in range(5):
            cy, cx, ry, rx = rs.randint(20, H - 20), rs.randint(20, W - 20), rs.randint(8, H // 4), rs.randint(8, W // 4)
            d = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
            masks[b][(d < 1) & (d > 0.25 * (b % 3))] = 1
        masks[b][rs.rand(H, W) < 0.01] ^= 1
    return masks


@pytest.mark.parametrize("H,W,n_frames", [(300, 260, 8), (480, 640, 3)])
def test_videos_above_the_old_limit_equal_the_host_composition(H, W, n_frames):
    frames, boxes = K.sequence(7 + H, n_frames, H, W)
    boxes[1] = (W // 2, H // 2, W + 30, H + 9)                        # leaves the frame
    assert H * W > lib().og_classic_limit(0)
    for src in (frames, np.ascontiguousarray(frames[..., 1])):
        e = CL.Classic(beta=0.7, percentile=30, n_components=2, chunk=2, tiled="auto")
        seed = e.init(src[:1], boxes[0])
        assert seed == CL.percentile_host(CL.box_hist_host(src[0], boxes[0]), 30)
        want = CL.guided_vft_host(src, boxes, seed)
        mask, area, th = e.guided_vft(src, boxes, want_thresh=True)
        assert np.array_equal(th.view(np.uint64), want[2].view(np.uint64))          # f64 thresholds bit for bit
        assert np.array_equal(area, want[1]) and np.array_equal(mask, np.stack(want[0]))
        assert e.thresh == want[3] and area.max() > 0
        e.thresh = seed
        none, only = e.guided_vft(src, boxes, want_mask=False)
        assert none is None and np.array_equal(only, want[1])
    off = CL.Classic()
    off.thresh = 100.0
    with pytest.raises(CL.OpenGlottalHipError, match="65536"):
        off.guided_vft(frames[:1], boxes[:1])


def test_otsu_above_the_old_limit():
    H, W = 480, 640
    frames, boxes = K.sequence(5, 3, H, W)
    boxes[2] = None
    e = CL.Classic(tiled="auto")
    for src in (frames, np.ascontiguousarray(frames[..., 1])):
        for want_mask in (True, False):
            mask, area, Tt = e.otsu_in_box(src, boxes, want_mask=want_mask)
            for i in range(3):
                g = bgr_to_gray(src[i]) if src[i].ndim == 3 else src[i]
                roi = K.roi_of(None if boxes[i] is None else normalize_box(boxes[i], W, H), H, W)
                t = K.otsu_numpy(CL.box_hist_host(src[i], boxes[i])) if boxes[i] is not None else 0
                want = ((g <= t) & roi) if boxes[i] is not None else np.zeros((H, W), bool)
                assert Tt[i] == t and area[i] == int(want.sum()), i
                if want_mask:
                    assert np.array_equal(mask[i], want.astype(np.uint8) * 255), i
            assert area[0] > 0 and area[2] == 0


def test_one_handle_across_modes_and_sizes():
    """96 x 96 (off), 300 x 260 (auto), 96 x 96 again, then 480 x 640 on ONE handle: each equal to a fresh handle's result and, through
    ``check``, to the references -- stale labels are never read and the workspace regrows in bytes."""
    small = np.stack([m for _, m in K.hard_masks(96)])
    e = fresh(2, "off")
    steps = [("96 off", "off", small, None), ("300x260 auto", "auto", blobby(3, 300, 260, 1), None),
             ("96 again", "auto", small, None), ("480x640 auto", "auto", blobby(2, 480, 640, 2), [(100, 60, 560, 470), (0, 0, 640, 480)])]
    for label, mode, batch, bx in steps:
        e.set_tiled(mode)
        got = TB.check(e, batch, bx, 2, label)
        want = TB.launch(fresh(2, mode), batch, bx)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), label
        assert got[1].min() > 0, label


# ── the Python surface ──────────────────────────────────────────────────────────
def test_features_and_tracker_on_a_300x260_clip():
    import openglottal_amd as og

    H, W, n = 300, 260, 10
    frames, boxes = K.sequence(23, n, H, W)
    init = 3
    p = F.YGVFT_PARAMS
    first = next(b for b in boxes[:init] if b is not None)
    seed = CL.percentile_host(CL.box_hist_host(frames[init - 1], first), p["glottal_percentile"])
    want = CL.guided_vft_host(frames[init:], boxes[init:], seed, p["beta"], p["glottal_percentile"], p["max_glottal_components"])
    feats = F.extract_features_yolo_guided_vft(frames, K.ScriptedDetector(boxes), init)
    assert np.array_equal(feats["_area"], [0.0] * init + [float(a) for a in want[1]]) and want[1].max() > 0
    tr = og.YOLOGuidedVFT(**p)
    tr.initialize(list(frames[:init]), bbox=first)
    assert tr.thresh == seed
    got = tr.process_frame(frames[init], boxes[init])
    assert np.array_equal(got, want[0][0])


def test_cli_guided_vft_on_a_480x640_clip(tmp_path, monkeypatch, capsys):
    """`--pipeline guided-vft` on a clip above the old limit returns features, and its areas are the host composition's."""
    import json

    import openglottal_amd
    from openglottal_amd import cli

    H, W, n = 480, 640, 6
    frames, boxes = K.sequence(31, n, H, W)
    np.save(tmp_path / "video.npy", frames)
    monkeypatch.setattr(openglottal_amd, "TemporalDetector", lambda path, **kw: K.ScriptedDetector(boxes))
    out = tmp_path / "out"
    rc = cli.main(["run", str(tmp_path / "video.npy"), "--pipeline", "guided-vft", "--yolo-weights", str(tmp_path / "yolo.npz"), "-o", str(out)])
    assert rc == 0 and "Features saved to" in capsys.readouterr().out
    got = json.load(open(out / "features.json"))
    init, p = F.YGVFT_INIT, F.YGVFT_PARAMS
    seed = CL.percentile_host(CL.box_hist_host(frames[init - 1], boxes[0]), p["glottal_percentile"])
    want = CL.guided_vft_host(frames[init:], boxes[init:], seed, p["beta"], p["glottal_percentile"], p["max_glottal_components"])
    assert got["_area"] == [0.0] * init + [float(v) for v in want[1]] and max(got["_area"]) > 0


# ── extents ─────────────────────────────────────────────────────────────────────
def test_extents_at_300x260_in_auto_mode():
    H, W, B, SEED = 300, 260, 3, 61.5
    frames, boxes = K.sequence(44, B, H, W)
    boxes[1] = (200, 250, 400, 400)                                  # leaves the frame
    bx = np.array([normalize_box(b, W, H) for b in boxes], np.int32)
    e = CL.Classic(chunk=2, tiled="auto")
    sync = lambda: check(lib().og_classic_sync(e._h), "og_classic_sync")
    same = lambda a, b: np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))
    for ch in (3, 1):
        src = frames if ch == 3 else np.ascontiguousarray(frames[..., 1])
        want = CL.guided_vft_host(src, boxes, SEED)
        wanted = {"mask": np.stack(want[0]), "area": want[1], "thresh": want[2]}
        for outs in (("mask", "area", "thresh"), ("area",)):
            sizes = {"mask": B * H * W if "mask" in outs else None, "area": 4 * B, "thresh": 8 * B if "thresh" in outs else None}

            def stream(p):
                check(lib().og_vft_guided_set_state(e._h, SEED))
                return lib().og_vft_guided_stream_u8(e._h, p["frames"], B, H, W, ch, p["boxes"], p["mask"], p["area"], p["thresh"])
            out = G.run_guarded("og_vft_guided_stream_u8", f"tiled ch={ch} outs={'+'.join(outs)}", stream, {"frames": src, "boxes": bx}, sizes)
            assert all(same(out[k], wanted[k]) for k in outs)

            def dev(p):
                check(lib().og_vft_guided_set_state(e._h, SEED))
                return lib().og_vft_guided_u8_dev(e._h, p["frames"], B, H, W, ch, p["boxes"], p["mask"], p["area"], p["thresh"])
            out = G.run_guarded("og_vft_guided_u8_dev", f"tiled ch={ch} outs={'+'.join(outs)}", dev, {"frames": src, "boxes": bx}, sizes,
                                "device", sync)
            assert all(same(out[k], wanted[k]) for k in outs)
        for want_mask in (True, False):
            sizes = {"mask": B * H * W if want_mask else None, "area": 4 * B, "T": 4 * B}
            out = G.run_guarded("og_otsu_in_box_u8", f"tiled ch={ch} mask={want_mask}",
                                lambda p: lib().og_otsu_in_box_u8(e._h, p["frames"], B, H, W, ch, p["boxes"], p["mask"], p["area"], p["T"]),
                                {"frames": src, "boxes": bx}, sizes)
            for i in range(B):
                assert out["T"].view(np.int32)[i] == CL.otsu_threshold_host(CL.box_hist_host(src[i], boxes[i]))


# ── the worst case ──────────────────────────────────────────────────────────────
def ladder_sides():
    sides, S = list(K.LADDER_SIDES), 512
    while S * S <= LIMIT:
        sides.append(S)
        S *= 2
    return sides


def test_worst_case_ladder_to_the_declared_limit():
    """The ladder of tests/test_gpu_classic_blobs.py with its rule unchanged, on the tiled path: S = 32 .. 256 with "always", then 512
    and upward, doubling to the declared limit.  A rung is launched only while the time predicted for it from the rungs before (the
    last time x max(4, the last growth)) stays under LADDER_LIMIT_S; otherwise the test FAILS without launching.  B = 1, gray, box =
    frame, n = 2, mask requested; one warm call, the median of three; a rung's time is its slowest mask."""
    import time

    sides = ladder_sides()
    assert sides[-1] ** 2 == LIMIT, "the declared limit is the last rung of the ladder"
    e = fresh(2, "always")
    times = []
    for S in sides:
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
            s_mask, s_area = K.scipy_blobs_cached(m, 2)
            h_mask, h_area = TB.host(m, 2)
            took = []
            for rep in range(4):
                out.fill_(7)
                area.fill_(-1)
                torch.cuda.synchronize()                                # the handle's stream does not wait for torch's
                t0 = time.perf_counter()
                e.guided_vft_dev(frames, 1, S, S, 1, bx, area, out, None)
                e.sync()
                took.append(time.perf_counter() - t0)
                assert int(area.cpu()[0]) == s_area == h_area, (name, S, rep)
                got = out.cpu().numpy()[0]
                assert np.array_equal(got, s_mask) and np.array_equal(got, h_mask), (name, S, rep)
            rung.append(float(np.median(took[1:])))
            print(f"tiled worst case {name} {S}x{S}: {rung[-1] * 1e3:.3f} ms (warm call {took[0] * 1e3:.3f} ms)")
        times.append(max(rung))
    print("tiled worst case per side (ms): " + ", ".join(f"{S}: {t * 1e3:.3f}" for S, t in zip(sides, times)))
    assert len(times) == len(sides)
