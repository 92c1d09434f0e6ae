"""-m gpu: the YOLO-Crop+UNet video pipeline (scripts/infer.py:222-248) streamed and compacted on the device
(`UNet.segment_crops_stream`, `features.crop_area_waveform`) against

* the host composition og_crop_tile_host -> `UNet.segment` -> og_crop_project_host (the kernels' own arithmetic on the host, itself
  judged against geometry.py in tests/test_crop_host.py), bit for bit;
* the staged evaluation path that existed before (`UNet.segment_crops`), bit for bit;
* itself under every way of cutting the video into micro-batches: a frame's result is a function of the frame and its box only.
"""
import numpy as np
import pytest

import crop_cases as K
import openglottal_amd as og
from openglottal_amd import evaluate, features, synth
from openglottal_amd.utils import bgr_to_gray

pytestmark = pytest.mark.gpu

FEATS = (4, 8, 16, 32)
B = 23


def _boxes(all_usable):
    if all_usable:
        return [K.USABLE[i % len(K.USABLE)] for i in range(B)]
    it = iter(range(10 ** 6))
    bx = [None if i % 3 == 2 else K.USABLE[next(it) % len(K.USABLE)] for i in range(B)]
    bx[4], bx[7] = K.SLIVER, K.EMPTY
    return bx


@pytest.fixture(scope="module")
def case():
    """The model, the video (BGR and its gray), both box sets and, computed once, the host composition of each."""
    m = og.UNet(1, 1, FEATS)
    m.load_state_dict(synth.make_unet_state_dict(FEATS, seed=11, head_scale=3.0, head_bias=0.5))
    m.to("cuda:0").eval()
    m.set_chunk(4)
    bgr = np.random.RandomState(31).randint(0, 256, (B, K.H, K.W, 3), dtype=np.uint8)
    gray = bgr_to_gray(bgr)
    c = {"m": m, "bgr": bgr, "gray": gray}
    for name, all_usable in (("mixed", False), ("all", True)):
        bx = _boxes(all_usable)
        rows = [(-1, -1, -1, -1) if b is None else b for b in bx]
        mask, area = K.host_composition(m, list(gray), rows, K.SIZE)
        c[name] = {"boxes": bx, "rows": rows, "mask": mask, "area": area}
    yield c
    m.set_chunk(32)


def test_mask_and_area_equal_the_host_composition(case):
    m = case["m"]
    for name in ("mixed", "all"):
        ref = case[name]
        mask, area = m.segment_crops_stream(case["gray"], ref["boxes"], crop_size=K.SIZE, want_mask=True)
        print(f"crop stream [{name}]: areas {area.tolist()}")
        assert np.array_equal(area, ref["area"]) and np.array_equal(mask, ref["mask"]), name
        assert np.array_equal(area, (mask > 0).sum((1, 2)))                                   # area == #(mask > 0)
        assert set(np.unique(mask).tolist()) == {0, 255} and (area > 0).sum() >= 8, name       # a real segmentation, both values
        for i, b in enumerate(ref["boxes"]):
            if b is None or b in (K.SLIVER, K.EMPTY):
                assert area[i] == 0 and not mask[i].any(), (name, i, b)
            else:
                x1, y1, x2, y2 = b
                outside = mask[i].copy()
                outside[y1:y2, x1:x2] = 0
                assert not outside.any(), (name, i, b)


def test_it_equals_the_staged_path_on_the_usable_boxes(case):
    m = case["m"]
    ref = case["mixed"]
    staged_boxes = [None if (b is None or b in (K.SLIVER, K.EMPTY)) else b for b in ref["boxes"]]     # (the staged entry refuses the sliver)
    staged = m.segment_crops(case["gray"], staged_boxes, crop_size=K.SIZE)
    assert np.array_equal(staged, ref["mask"])
    staged = m.segment_crops(case["gray"], case["all"]["boxes"], crop_size=K.SIZE)
    assert np.array_equal(staged, case["all"]["mask"])


def test_the_same_bits_however_the_video_is_cut_and_fed(case):
    m = case["m"]
    for name in ("mixed", "all"):
        ref = case[name]
        try:
            for chunk in (1, 4, 32):
                m.set_chunk(chunk)
                for lanes in (1, 0):
                    m.set_option("lanes", lanes)
                    mask, area = m.segment_crops_stream(case["gray"], ref["boxes"], crop_size=K.SIZE, want_mask=True)
                    assert np.array_equal(area, ref["area"]) and np.array_equal(mask, ref["mask"]), (name, chunk, lanes)
        finally:
            m.set_option("lanes", 0)
            m.set_chunk(4)
        # BGR frames whose gray the gray frames are; a list of frames; want_mask off; an int32 array of normalised rows as boxes
        mask, area = m.segment_crops_stream(case["bgr"], ref["boxes"], crop_size=K.SIZE, want_mask=True)
        assert np.array_equal(area, ref["area"]) and np.array_equal(mask, ref["mask"]), name
        for frames in (list(case["bgr"]), list(case["gray"]), [f.copy() for f in case["gray"]]):
            mask, area = m.segment_crops_stream(frames, ref["boxes"], crop_size=K.SIZE, want_mask=True)
            assert np.array_equal(area, ref["area"]) and np.array_equal(mask, ref["mask"]), name
        none, area = m.segment_crops_stream(case["bgr"], np.array(ref["rows"], np.int32), crop_size=K.SIZE)
        assert none is None and np.array_equal(area, ref["area"]), name


def test_resident_frames_through_the_dev_entry(case):
    import torch

    m = case["m"]
    ref = case["mixed"]
    rows = torch.from_numpy(np.array(ref["rows"], np.int32)).cuda()
    for src, ch in ((case["gray"], 1), (case["bgr"], 3)):
        d_src = torch.from_numpy(src).cuda()
        tiles = torch.empty((B, K.SIZE, K.SIZE), dtype=torch.uint8, device="cuda")
        tmask = torch.empty_like(tiles)
        mask = torch.empty((B, K.H, K.W), dtype=torch.uint8, device="cuda")
        area = torch.empty(B, dtype=torch.int32, device="cuda")
        area2 = torch.empty(B, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        m.segment_crops_dev(d_src, B, K.H, K.W, ch, rows, K.SIZE, tiles, tmask, area_dev=area, mask_dev=mask)
        m.segment_crops_dev(d_src, B, K.H, K.W, ch, rows, K.SIZE, tiles, tmask, area_dev=area2)        # the box-walk count, no mask
        m.sync()
        assert np.array_equal(area.cpu().numpy(), ref["area"]) and np.array_equal(area2.cpu().numpy(), ref["area"]), ch
        assert np.array_equal(mask.cpu().numpy(), ref["mask"]), ch
        want_tiles = np.stack([K.tile_host(f, b, K.SIZE) for f, b in zip(case["gray"], ref["rows"])])
        assert np.array_equal(tiles.cpu().numpy(), want_tiles), ch


def test_full_width_net_at_256_equals_the_staged_path():
    feats = (32, 64, 128, 256)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5))
    m.to("cuda:0").eval()
    gray = synth.random_gray_frames(6, 256, 256, seed=9)
    boxes = [(0, 0, 256, 256), (40, 30, 200, 250), None, (100, 90, 140, 150), (3, 0, 4, 250), (0, 128, 256, 256)]
    staged = m.segment_crops(gray, boxes, crop_size=256)
    mask, area = m.segment_crops_stream(gray, boxes, crop_size=256, want_mask=True)
    assert np.array_equal(mask, staged) and np.array_equal(area, (staged > 0).sum((1, 2)))
    assert area[2] == 0 and set(np.unique(mask).tolist()) == {0, 255}
    _, area2 = m.segment_crops_stream(gray, boxes, crop_size=256)
    assert np.array_equal(area2, area)


def test_f16_mode_succeeds_and_stays_a_function_of_the_frame(case):
    m = case["m"]
    ref = case["mixed"]
    try:
        m.set_option("precision", 2)
        _, want = K.host_composition(m, list(case["gray"]), ref["rows"], K.SIZE)         # through the same f16 handle
        for chunk in (4, 1):
            m.set_chunk(chunk)
            _, area = m.segment_crops_stream(case["bgr"], ref["boxes"], crop_size=K.SIZE)
            assert np.array_equal(area, want), chunk
    finally:
        m.set_option("precision", 0)
        m.set_chunk(4)
    _, area = m.segment_crops_stream(case["bgr"], ref["boxes"], crop_size=K.SIZE)
    assert np.array_equal(area, ref["area"])


def _scripted_detector(script):
    calls = {"i": 0}

    def backend(frame, conf):
        d = [x for x in script[calls["i"]] if x[4] >= conf]
        calls["i"] += 1
        return (np.array([x[:4] for x in d], np.float32).reshape(-1, 4), np.array([x[4] for x in d], np.float32))

    return og.TemporalDetector(backend), calls


def test_crop_area_waveform_equals_the_per_frame_loop(case):
    """A scripted detector backend, as the trace tests of tests/test_host_logic.py build theirs: hits, three misses (held), a
    fourth miss (the box is dropped), a new hit, a jump (treated as a miss: held), hits again."""
    m = case["m"]
    hit = lambda x, y: [[x, y, x + 30.0, y + 24.0, 0.9]]
    script = ([hit(20 + i, 15 + i) for i in range(10)] + [[]] * 3 + [hit(31, 26)] + [[]] * 4 + [[]] + [hit(50, 40)] +
              [hit(5, 5)] + [hit(52 + i, 41) for i in range(6)] + [[[10, 10, 20, 20, 0.1]]] + [hit(55, 40 - i) for i in range(12)])
    assert len(script) == 40
    video = np.random.RandomState(32).randint(0, 256, (40, K.H, K.W, 3), dtype=np.uint8)
    det, calls = _scripted_detector(script)
    want, boxes = [], []
    for frm in video:
        box = det.detect(frm)
        boxes.append(box)
        want.append(0.0 if box is None else float(np.sum(evaluate.unet_on_crop(bgr_to_gray(frm), box, m, crop_size=K.SIZE) > 0)))
    assert sum(b is None for b in boxes) >= 2 and boxes[17] is None and boxes[12] is not None and boxes[20] == boxes[19]
    det2, calls2 = _scripted_detector(script)
    det2.detect(video[0])            # stale state: crop_area_waveform resets the detector
    calls2["i"] = 0
    wave = features.crop_area_waveform(video, det2, m, crop_size=K.SIZE)
    assert calls2["i"] == 40 and wave.dtype == np.float64
    assert np.array_equal(wave, np.array(want)) and wave.max() > 0
    calls2["i"] = 0
    assert np.array_equal(features.crop_area_waveform(list(video), det2, m, crop_size=K.SIZE), wave)      # a list of frames


def _infer_loop_area(gray, box, m, size):
    """The loop body of infer.py:230-246, literally, in numpy (geometry.py) around a device call on the tile."""
    from openglottal_amd import geometry

    if box is None:
        return 0.0
    x1, y1, x2, y2 = box
    crop = gray[y1:y2, x1:x2]
    if crop.size == 0:
        return 0.0
    boxed, pad_t, pad_l, content_h, content_w = geometry.letterbox_with_info(crop, size, value=0)
    mask_cs = m.segment(boxed[None], want_area=False)[0][0]
    mask_orig = geometry.unletterbox(mask_cs, pad_t, pad_l, content_h, content_w, crop.shape[0], crop.shape[1])
    return float(np.sum(mask_orig > 0))


def test_crop_area_waveform_over_the_native_detector_backend(case):
    """The native backend (`detect_frames`): detector network and state machine of block k + 1 run on the worker thread under the
    crop pass of block k (`_blocks_with_boxes`, unchanged).  150 frames are two blocks.  Expected: the batched raw detections replayed
    through the state machine, then the reference's loop body per frame.  The seeded detector reports boxes taller than the 80-row
    frame, so `TemporalDetector` returns some with y1 < 0: `gray[y1:y2, x1:x2]` then counts from the END of the axis, and so must
    the streamed pass (`utils.normalize_box`; the staged `segment_crops` clamps such a box to the frame instead)."""
    from openglottal_amd.yolo import YoloV8Detector

    m = case["m"]
    d = YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0")
    conf = 0.001       # seeded weights on noise: low enough that the detector reports boxes
    video = np.random.RandomState(34).randint(0, 256, (150, K.H, K.W, 3), dtype=np.uint8)
    best = d.detect_frames(video, conf)
    td = og.TemporalDetector(lambda f, c: None, conf=conf)
    boxes = [td.update(b[None, :4], b[4:5], K.W, K.H) if b[4] >= 0 else td.update(None, None, K.W, K.H) for b in best]
    assert sum(b is not None for b in boxes) >= 10 and any(b is not None and min(b) < 0 for b in boxes)
    want = [_infer_loop_area(bgr_to_gray(frm), box, m, K.SIZE) for frm, box in zip(video, boxes)]
    wave = features.crop_area_waveform(video, og.TemporalDetector(d, conf=conf), m, crop_size=K.SIZE)
    print(f"crop waveform over the native detector: {sum(b is not None for b in boxes)} boxes, {int((wave > 0).sum())} frames with area")
    assert np.array_equal(wave, np.array(want))


def test_extract_features_unet_crop(case):
    m = case["m"]
    video = np.random.RandomState(33).randint(0, 256, (12, K.H, K.W, 3), dtype=np.uint8)
    det, _ = _scripted_detector([[]] * 12)
    assert og.extract_features_unet_crop(video, det, m) is None                    # no detections: an all-zero waveform
    assert og.extract_features_unet_crop(video[:0], det, m) is None                # an empty video
    script = [[[30.0 + i, 20.0, 60.0 + i, 50.0, 0.9]] for i in range(12)]
    det, _ = _scripted_detector(script)
    f = og.extract_features_unet_crop(video, det, m)                               # (the reference's tile side, 256)
    det, _ = _scripted_detector(script)
    wave = features.crop_area_waveform(video, det, m)
    want = features._kinematic_features([float(v) for v in wave])
    assert f is not None and wave.max() > 0 and np.array_equal(f["_area"], wave)
    assert all(f[k] == want[k] for k in want if k != "_area")
