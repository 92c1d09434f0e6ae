"""-m gpu: `infer.run_pipeline` for its four pipelines against what the project already has: the areas equal the existing
waveform functions bit for bit, the frames equal `overlay.draw_overlay` applied frame by frame to the masks and boxes the existing
host-returning entries give, and the Python detector is left in the state the existing pass leaves it in.  12 frames at 256 x 256
(network size) and 12 at 96 x 80 (the resized entries), a stretch of None boxes and the seed frames of guided-vft among them."""
import numpy as np
import pytest

import crop_cases as K
import openglottal_amd as og
from openglottal_amd import classic as CL
from openglottal_amd import features as F
from openglottal_amd import infer as I
from openglottal_amd import overlay as OV
from openglottal_amd import synth
from openglottal_amd.utils import NET_SIZE, bgr_to_gray, normalize_box

pytestmark = pytest.mark.gpu

FEATS = (4, 8, 16, 32)
N = 12
hit = lambda x, y: [[x, y, x + 30.0, y + 24.0, 0.9]]
# hits, four misses (three held, then the box is dropped: two frames of None), new hits
SCRIPT = [hit(20 + i, 15 + i) for i in range(3)] + [[]] * 5 + [hit(31 + i, 26) for i in range(4)]
SHAPES = ((256, 256), (K.H, K.W))


def scripted():
    calls = {"i": 0}

    def backend(frame, conf):
        d = [x for x in SCRIPT[calls["i"]] if x[4] >= conf]
        calls["i"] += 1
        return (np.array([x[:4] for x in d], np.float32).reshape(-1, 4), np.array([x[4] for x in d], np.float32))

    return og.TemporalDetector(backend), calls


def state(det):
    return {k: (None if v is None else np.asarray(v).tolist()) for k, v in vars(det).items() if k != "model" and not callable(v)}


@pytest.fixture(scope="module")
def model():
    m = og.UNet(1, 1, FEATS)
    m.load_state_dict(synth.make_unet_state_dict(FEATS, seed=11, head_scale=3.0, head_bias=0.5))
    m.to("cuda:0").eval()
    m.set_chunk(4)
    return m


def video(H, W):
    return np.random.RandomState(H + 3 * W).randint(0, 256, (N, H, W, 3), dtype=np.uint8)


def boxes_of(v):
    det, _ = scripted()
    bx = [det.detect(f) for f in v]
    assert bx[0] is not None and bx[5] is not None and bx[6] is None and bx[7] is None and bx[8] is not None      # held, then dropped
    return bx, state(det)


def full_masks(model, v):
    H, W = v.shape[1:3]
    if (H, W) == (NET_SIZE, NET_SIZE):
        return model.segment(bgr_to_gray(v), want_area=False)[0]
    return model.segment_resized(v, net=NET_SIZE, want_mask=True)[0]


def check(v, got, masks, boxes, style):
    frames, _ = got
    assert frames.shape == v.shape and frames.dtype == np.uint8
    for i in range(N):
        want = OV.draw_overlay(v[i], masks[i], boxes[i], 0.0, overlay_style=style)
        assert np.array_equal(frames[i], want), (style, i)


@pytest.mark.parametrize("H,W", SHAPES)
def test_unet_and_unet_only(model, H, W):
    v = video(H, W)
    boxes, end = boxes_of(v)
    full = full_masks(model, v)
    assert full.any()
    det, calls = scripted()
    wave = F.area_waveform(v, det, model)
    assert state(det) == end
    for style in ("fill", "contour", "none"):
        det2, calls2 = scripted()
        det2.detect(v[0])                                                 # stale state: run_pipeline resets the detector
        calls2["i"] = 0
        got = I.run_pipeline(v, det2, "unet", model, "cuda:0", overlay_style=style)
        assert calls2["i"] == N and state(det2) == end
        assert got[1].dtype == np.float64 and np.array_equal(got[1], wave) and wave.max() > 0
        check(v, got, [None if b is None else m for m, b in zip(full, boxes)], boxes, style)      # the FULL mask, not cut to the box
    only = F.area_waveform(v, None, model)
    got = I.run_pipeline(v, None, "unet-only", model, "cuda:0")
    assert np.array_equal(got[1], only) and np.array_equal(only, (full > 0).sum((1, 2)))
    check(v, got, full, [None] * N, "fill")
    got = I.run_pipeline(list(v), None, "unet-only", model, "cuda:0", overlay_style="contour")    # a list of frames
    check(v, got, full, [None] * N, "contour")


@pytest.mark.parametrize("H,W", SHAPES)
def test_yolo_crop_unet(model, H, W):
    v = video(H, W)
    boxes, end = boxes_of(v)
    masks, area = model.segment_crops_stream(v, boxes, crop_size=K.SIZE, want_mask=True)
    det, _ = scripted()
    wave = F.crop_area_waveform(v, det, model, crop_size=K.SIZE)
    assert np.array_equal(wave, area) and wave.max() > 0 and state(det) == end
    det2, calls2 = scripted()
    got = I.run_pipeline(v, det2, "yolo-crop+unet", model, "cuda:0", crop_size=K.SIZE)
    assert calls2["i"] == N and state(det2) == end and np.array_equal(got[1], wave)
    check(v, got, [None if b is None else m for m, b in zip(masks, boxes)], boxes, "fill")        # the pasted crop mask


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("init", (2, 7))
def test_guided_vft(H, W, init):
    """init 7: the first box is seen, the seed frames end inside the stretch of None boxes."""
    v = video(H, W)
    v[:, H // 4:H // 2, W // 4:W // 2] //= 4                              # something dark to segment
    boxes, end = boxes_of(v)
    det, _ = scripted()
    wave = F.guided_vft_area_waveform(v, det, ygvft_init=init)
    assert state(det) == end and not wave[:init].any() and wave.max() > 0
    e = CL.Classic(tiled="auto")
    first = next((b for b in boxes[:init] if b is not None), None)
    e.init([v[init - 1]], None if first is None else normalize_box(first, W, H))
    masks, area = e.guided_vft(v[init:], boxes[init:])
    assert np.array_equal(wave[init:], area)
    det2, calls2 = scripted()
    for style in ("fill", "contour"):
        calls2["i"] = 0
        got = I.run_pipeline(v, det2, "guided-vft", None, "cuda:0", overlay_style=style, ygvft_init=init)
        assert calls2["i"] == N and state(det2) == end and np.array_equal(got[1], wave)
        check(v, got, [None] * init + list(masks), boxes, style)          # seed frames: no mask, the box is still drawn


def test_a_video_shorter_than_the_seed_and_an_empty_one():
    whole = video(K.H, K.W)
    v = whole[:1]
    det, _ = scripted()
    got = I.run_pipeline(v, det, "guided-vft", None, "cuda:0")
    assert np.array_equal(got[1], [0.0]) and np.array_equal(got[0][0], OV.draw_overlay(v[0], None, boxes_of(whole)[0][0], 0))
    det, _ = scripted()
    frames, wave = I.run_pipeline(v[:0], det, "guided-vft", None, "cuda:0")
    assert len(frames) == 0 and len(wave) == 0
