"""-m gpu: YOLO+Otsu on the device (og_otsu_in_box_u8 / _dev) against the host twins on 70 frames of 48 x 32, empty and
out-of-frame boxes included.  Equality everywhere."""
import numpy as np
import pytest
import torch

from openglottal_amd import classic as CL
from openglottal_amd.utils import bgr_to_gray_numpy, normalize_box

pytestmark = pytest.mark.gpu

B, H, W = 70, 32, 48


def inputs():
    rs = np.random.RandomState(17)
    bgr = rs.randint(0, 256, (B, H, W, 3), dtype=np.uint8)
    bgr[:, 10:22, 14:34] //= 4                                  # a dark region: a bimodal ROI
    bgr[3] = 90                                                 # a constant frame: no threshold qualifies, T = 0
    boxes = []
    for i in range(B):
        x1, y1 = rs.randint(0, 20), rs.randint(0, 12)
        boxes.append((x1, y1, x1 + rs.randint(8, 28), y1 + rs.randint(6, 20)))
    boxes[1] = None
    boxes[5] = (20, 10, 20, 25)                                 # empty
    boxes[6] = (60, 40, 90, 70)                                 # outside the frame
    boxes[7] = (40, 25, 80, 60)                                 # leaves the frame
    boxes[8] = (-10, -8, -2, -1)                                # counted from the far edge
    boxes[9] = (11, 11, 12, 12)                                 # a single pixel
    boxes[10] = (0, 0, W, H)
    return bgr, boxes


def host(gray, boxes):
    masks = np.zeros((B, H, W), np.uint8)
    areas, Ts = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for i, b in enumerate(boxes):
        x1, y1, x2, y2 = normalize_box(b, W, H)
        h = CL.box_hist_host(gray[i], b)
        if x1 < 0 or not h.any():
            continue
        Ts[i] = CL.otsu_threshold_host(h)
        masks[i, y1:y2, x1:x2] = (gray[i, y1:y2, x1:x2] <= Ts[i]) * 255
        areas[i] = int((masks[i] > 0).sum())
    return masks, areas, Ts


def test_otsu_in_box_equals_the_host_twin():
    bgr, boxes = inputs()
    gray = bgr_to_gray_numpy(bgr)
    want = host(gray, boxes)
    assert want[2][3] == 0 and want[1][[1, 5, 6]].sum() == 0 and want[1][7] > 0 and want[2][9] == 0      # (one pixel: no split qualifies)
    e = CL.Classic()
    for chunk in (32, 3):
        e.set_chunk(chunk)
        for src in (gray, bgr):
            mask, area, T = e.otsu_in_box(src, boxes)
            assert np.array_equal(T, want[2]) and np.array_equal(area, want[1]) and np.array_equal(mask, want[0]), (chunk, src.ndim)
            mask, area, T = e.otsu_in_box(src, boxes, want_mask=False)
            assert mask is None and np.array_equal(T, want[2]) and np.array_equal(area, want[1])
    # resident
    src = torch.from_numpy(bgr).cuda()
    bx = torch.from_numpy(np.array([normalize_box(b, W, H) for b in boxes], np.int32)).cuda()
    mask = torch.full((B, H, W), 9, dtype=torch.uint8, device="cuda")
    area = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    T = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    e.otsu_in_box_dev(src, B, H, W, 3, bx, area, T, mask)
    e.sync()
    assert np.array_equal(T.cpu().numpy(), want[2]) and np.array_equal(area.cpu().numpy(), want[1])
    assert np.array_equal(mask.cpu().numpy(), want[0])


class _Replay:
    """A detector that replays one box per call; ``reset`` keeps the position (evaluate resets at every patient change)."""
    model = None

    def __init__(self, boxes):
        self.boxes, self.i = list(boxes), 0

    def reset(self):
        pass

    def detect(self, frame):
        self.i += 1
        return self.boxes[self.i - 1]


def test_evaluate_classical_rows_equal_a_host_composition_and_the_default_is_unchanged():
    import classic_cases as K
    import openglottal_amd as og
    from openglottal_amd import evaluate as E
    from openglottal_amd import synth
    from openglottal_amd.features import YGVFT_INIT
    from openglottal_amd.utils import frame_metrics

    feats = (4, 8, 16, 32)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=11, head_scale=3.0, head_bias=0.5))
    m.to("cuda:0").eval()
    fa, ba = K.sequence(71, 9, 64, 64)
    fb, bb = K.sequence(72, 7, 64, 64)
    fc, bc = K.sequence(73, 2, 64, 64)                          # a patient with init frames only: counted, never scored
    frames, boxes = np.concatenate([fa, fb, fc]), ba + bb + bc
    boxes[0] = None                                            # the first box of patient a is seen on its second frame
    patients = ["a"] * 9 + ["b"] * 7 + ["c"] * 2
    gray = bgr_to_gray_numpy(frames)
    gts = ((gray < 60) * 255).astype(np.uint8)
    n = len(frames)

    plain = E.evaluate(frames, gts, m, detector=_Replay(boxes), patients=patients)
    again = E.evaluate(frames, gts, m, detector=_Replay(boxes), patients=patients, classical=False)
    assert list(plain[0]) == E.PIPELINES and plain[0] == again[0] and plain[1] == again[1] and plain[2] == again[2]
    agg, per_patient, det = E.evaluate(frames, gts, m, detector=_Replay(boxes), patients=patients, classical=True)
    assert list(agg) == ["unet-only", "yolo+otsu", "yolo+unet", "yolo-crop+unet", "yolo+motion"]
    for p in E.PIPELINES:
        assert agg[p] == plain[0][p]
    assert det == plain[2]

    want_o = {"dice": [], "iou": []}
    for i in range(n):
        x1, y1, x2, y2 = normalize_box(boxes[i], 64, 64)
        mk = np.zeros((64, 64), np.uint8)
        h = CL.box_hist_host(gray[i], boxes[i])
        if h.any():
            mk[y1:y2, x1:x2] = (gray[i, y1:y2, x1:x2] <= CL.otsu_threshold_host(h)) * 255
        d, j = frame_metrics(mk, gts[i])
        want_o["dice"].append(d)
        want_o["iou"].append(j)
    n_det = sum(b is not None for b in boxes)
    assert agg["yolo+otsu"] == {"dice": want_o["dice"], "iou": want_o["iou"], "n_det": n_det, "n_total": n}

    want_m = {"dice": [], "iou": []}
    for lo, hi in ((0, 9), (9, 16)):
        first = next((b for b in boxes[lo:lo + YGVFT_INIT] if b is not None), None)
        hh = CL.box_hist_host(gray[lo + YGVFT_INIT - 1], first)
        if not hh.any():
            hh = CL.box_hist_host(gray[lo + YGVFT_INIT - 1], (0, 0, 64, 64))
        masks, _, _, _ = CL.guided_vft_host(gray[lo + YGVFT_INIT:hi], boxes[lo + YGVFT_INIT:hi], CL.percentile_host(hh, 30))
        for k, mk in enumerate(masks):
            d, j = frame_metrics(mk, gts[lo + YGVFT_INIT + k])
            want_m["dice"].append(d)
            want_m["iou"].append(j)
    assert agg["yolo+motion"] == {"dice": want_m["dice"], "iou": want_m["iou"], "n_det": n_det, "n_total": n}
    assert len(want_m["dice"]) == n - 3 * YGVFT_INIT and "yolo+motion" not in per_patient["c"]
    assert per_patient["a"]["yolo+motion"] == want_m["dice"][:7] and per_patient["b"]["yolo+otsu"] == want_o["dice"][9:16]
    assert "yolo+otsu" in E.summarize(agg) and E.summarize(agg)["yolo+motion"]["n"] == n
    E.print_table(agg)
