"""-m gpu: the guided-VFT pass on the device (og_vft_guided_stream_u8 and its siblings) against the fixture the reference's own
YOLOGuidedVFT wrote (tests/golden/vft_guided.npz): areas, thresholds bit for bit, masks; gray and BGR, an array and a list of
frames, mask on and off, micro-batches of 1, 4 and 32 frames (the threshold is carried across them on the device), the per-frame
``YOLOGuidedVFT.process_frame`` loop, the resident entry, and ``extract_features_yolo_guided_vft``.  Equality everywhere."""
import numpy as np
import pytest
import torch

import classic_cases as K
import openglottal_amd as og
from openglottal_amd import classic as CL
from openglottal_amd import features as F
from openglottal_amd.utils import bgr_to_gray_numpy, normalize_box

pytestmark = pytest.mark.gpu

GOLD = K.golden()


def first_box(g):
    return next((b for b in g["boxes"][:g["init"]] if b is not None), None)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("name", sorted(GOLD))
def test_streamed_pass_equals_the_fixture(name):
    g = GOLD[name]
    init, boxes = g["init"], g["boxes"][g["init"]:]
    bgr = g["frames"]
    gray = bgr_to_gray_numpy(bgr)
    assert any(b is None for b in boxes) and any(b is not None and b[0] < 0 for b in boxes)
    e = CL.Classic()
    for chunk in (1, 4, 32):
        e.set_chunk(chunk)
        for src in (gray, bgr):
            for as_list in (False, True):
                for want_mask in (True, False):
                    seed = e.init(list(src[:init]) if as_list else src[:init], first_box(g))
                    assert same_bits(seed, g["seed"])
                    rest = list(src[init:]) if as_list else src[init:]
                    mask, area, th = e.guided_vft(rest, boxes, want_mask=want_mask, want_thresh=True)
                    label = (name, chunk, src.ndim, as_list, want_mask)
                    assert np.array_equal(area, g["area"]), label
                    assert same_bits(th, g["thresh"]), label
                    assert (mask is None) if not want_mask else np.array_equal(mask, g["masks"]), label
                    assert same_bits(e.thresh, g["thresh"][-1]), label


@pytest.mark.parametrize("name", sorted(GOLD))
def test_per_frame_tracker_and_resident_entry_equal_the_fixture(name):
    g = GOLD[name]
    init, boxes = g["init"], g["boxes"][g["init"]:]
    gray = bgr_to_gray_numpy(g["frames"])
    tr = og.YOLOGuidedVFT(**F.YGVFT_PARAMS)
    assert tr.thresh is None and tr.lmap is None
    tr.initialize(list(gray[:init]), bbox=first_box(g))
    assert same_bits(tr.thresh, g["seed"])
    for i, (f, b) in enumerate(zip(gray[init:], boxes)):
        m = tr.process_frame(f, b)
        assert m.dtype == np.uint8 and np.array_equal(m, g["masks"][i]), (name, i)
        assert same_bits(tr.thresh, g["thresh"][i]), (name, i)
    from openglottal_amd.models.tracker import YOLOGuidedVFT as ByModelsPath
    assert ByModelsPath is og.YOLOGuidedVFT
    # resident: BGR frames, boxes and outputs on the device, micro-batches of 4
    e = CL.Classic(chunk=4)
    e.thresh = g["seed"]
    B, H, W = gray.shape[0] - init, gray.shape[1], gray.shape[2]
    src = torch.from_numpy(g["frames"][init:].copy()).cuda()
    bx = torch.from_numpy(np.array([normalize_box(b, W, H) for b in boxes], np.int32)).cuda()
    mask = torch.full((B, H, W), 9, dtype=torch.uint8, device="cuda")
    area = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    th = torch.zeros(B, dtype=torch.float64, device="cuda")
    e.guided_vft_dev(src, B, H, W, 3, bx, area, mask, th)
    e.sync()
    assert np.array_equal(area.cpu().numpy(), g["area"]) and np.array_equal(mask.cpu().numpy(), g["masks"])
    assert same_bits(th.cpu().numpy(), g["thresh"])


def test_none_run_small_box_and_host_composition():
    """A run of None boxes still runs the recurrence; a box of 9 pixels keeps the threshold as its own input; the device equals the
    host composition on a sequence the fixture does not hold (48 x 32, 21 frames, chunk 4: five micro-batch boundaries)."""
    frames, boxes = K.sequence(91, 21, 32, 48)
    H, W = 32, 48
    seed = CL.percentile_host(CL.box_hist_host(frames[1], boxes[0]), 30)
    want = CL.guided_vft_host(frames[2:], boxes[2:], seed)
    e = CL.Classic(chunk=4)
    assert same_bits(e.init(frames[:2], boxes[0]), seed)
    mask, area, th = e.guided_vft(frames[2:], boxes[2:], want_thresh=True)
    assert np.array_equal(area, want[1]) and same_bits(th, want[2]) and np.array_equal(mask, np.stack(want[0]))
    none_run = [i for i, b in enumerate(boxes[2:]) if b is None]
    assert len(none_run) >= 3 and not area[none_run].any()
    for i in none_run:                                                                               # the recurrence was not skipped
        assert same_bits(th[i], 0.7 * float(th[i - 1]) + (1 - 0.7) * float(th[i - 1])), i
    x1, y1, x2, y2 = boxes[14]
    assert (x2 - x1) * (y2 - y1) <= 10
    t_before = float(th[14 - 2 - 1])
    assert same_bits(th[14 - 2], 0.7 * t_before + (1 - 0.7) * t_before)


def test_stream_without_a_threshold_is_refused_and_the_handle_stays_usable():
    e = CL.Classic()
    f = np.zeros((2, 8, 8), np.uint8)
    with pytest.raises(og.OpenGlottalHipError, match="no running threshold"):
        e.guided_vft(f, [None, None])
    e.thresh = 50.0
    _, area = e.guided_vft(f, [(0, 0, 8, 8), None])
    assert area.tolist() == [64, 0]
    e.reset(0.7, 30, 2)
    with pytest.raises(og.OpenGlottalHipError, match="no running threshold"):
        e.guided_vft(f, [None, None])


@pytest.mark.parametrize("name", sorted(GOLD))
def test_extract_features_equals_the_fixture(name):
    g = GOLD[name]
    feats = F.extract_features_yolo_guided_vft(g["frames"], K.ScriptedDetector(g["boxes"]), g["init"])
    assert np.array_equal(feats["_area"], [0.0] * g["init"] + [float(a) for a in g["area"]])
    assert [k for k in feats if k != "_area"] == list(g["feats"])
    for k, v in g["feats"].items():
        assert (feats[k] is None) if v is None else same_bits(feats[k], v), (name, k)
    as_list = F.extract_features_yolo_guided_vft(list(g["frames"]), K.ScriptedDetector(g["boxes"]), g["init"])
    assert np.array_equal(as_list["_area"], feats["_area"])
    assert F.extract_features_yolo_guided_vft(g["frames"][:g["init"] + 1], K.ScriptedDetector(g["boxes"]), g["init"]) is None


def test_one_handle_across_frame_sizes():
    """Many small frames, then a few large ones, then small ones again on ONE handle (the workspace is kept in bytes of the
    micro-batch and regrown in between): every pass equals the host composition."""
    e = CL.Classic(chunk=64)
    for seed, n, H, W in ((5, 40, 17, 23), (6, 3, 256, 256), (7, 40, 17, 23), (8, 9, 120, 160)):
        frames, boxes = K.sequence(seed, n, H, W)
        e.thresh = 70.0
        want = CL.guided_vft_host(frames, boxes, 70.0)
        mask, area, th = e.guided_vft(frames, boxes, want_thresh=True)
        assert np.array_equal(area, want[1]) and same_bits(th, want[2]) and np.array_equal(mask, np.stack(want[0])), (H, W)
        e.thresh = 70.0
        assert np.array_equal(e.guided_vft(frames, boxes, want_mask=False)[1], want[1]), (H, W)      # areas only: the window-only count
    with pytest.raises(og.OpenGlottalHipError, match="65536"):
        e.guided_vft(np.zeros((1, 257, 256), np.uint8), [None])
