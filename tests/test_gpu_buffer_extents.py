"""-m gpu: every entry point held to the buffer extents its caller declared (tests/buffer_guard.py).

The other GPU tests compare what the kernels compute; this module checks WHERE they write and WHICH bytes a result depends on.
Every entry is called through the raw C-ABI on `[guard | payload | guard]` outputs and `[slack | payload | slack]` inputs:
guards untouched, every declared byte written, results independent of the slack (0x00 / 0xFF), inputs unchanged, and the
payloads bit-identical to the same call on plain buffers (and to the Python wrapper where one exists).

The dimensions of each test are crossed in full, with two exceptions that alternate from case to case instead: boxes NULL / given
in the U-Net chain, and which outputs are NULL (three such calls on three of the 18 (B, chunk, lanes) triples per net and option set).
"""
import ctypes as C
import itertools
import time

import numpy as np
import pytest

import buffer_guard as G
import openglottal_amd as og
from openglottal_amd import synth
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

T0 = [0.0]      # set by the module's first test
OG_EINVAL = -1
FULL = (32, 64, 128, 256)
CONF = 0.001

# entry point -> the test(s) of this module that put it inside guards (tests/test_buffer_guard.py checks this table against the header)
MATRIX = {
    "og_unet_segment_u8_dev": "test_unet_chain",
    "og_unet_segment_u8": "test_unet_chain",
    "og_unet_segment_resized_u8_dev": "test_resized_path",
    "og_unet_stream_resized_u8": "test_resized_path",
    "og_unet_stream_frames_resized_u8": "test_resized_path",
    "og_mask_area_dev": "test_mask_area_and_stats",
    "og_mask_stats_dev": "test_mask_area_and_stats",
    "og_bgr2gray_dev": "test_a_positive_control_bgr2gray_overrun_is_reported test_bgr2gray_dev",
    "og_canvas_letterbox_u8_dev": "test_canvas_letterbox",
    "og_canvas_letterbox_u8": "test_canvas_letterbox",
    "og_unet_segment_crops_u8_dev": "test_segment_crops",
    "og_unet_segment_crops_u8": "test_segment_crops",
    "og_yolo_detect_u8_dev": "test_detector",
    "og_yolo_detect_u8": "test_detector test_detector_zero_copy_and_begin_end",
    "og_yolo_detect_u8_begin": "test_detector_zero_copy_and_begin_end",
    "og_yolo_detect_u8_end": "test_detector_zero_copy_and_begin_end",
    "og_yolo_detect_resized_u8_begin": "test_detector_zero_copy_and_begin_end",
    "og_yolo_letterbox_u8_dev": "test_yolo_letterbox_dev",
    "og_yolo_detect_resized_u8_dev": "test_detector_resized",
    "og_yolo_detect_resized_u8": "test_detector_resized",
    "og_unet_stream_u8": "test_host_streaming_and_zero_copy",
    "og_unet_stream_frames_u8": "test_host_streaming_and_zero_copy",
    "og_unet_forward_f32": "test_parity_entries",
    "og_unet_get_activation": "test_parity_entries",
    "og_yolo_get_activation": "test_parity_entries",
}

DEFAULTS = {"splitk": 0, "precision": 0, "wino": 1, "conv_impl": 2, "splitk_fused": 1, "wino_w": 1, "fuse_head": 1, "fuse_first": 1,
            "lanes": 0, "zero_copy": 1}
OPTION_SETS = [
    ("default", {}),
    ("wino=0", {"wino": 0}),
    ("wino=0,conv_impl=0", {"wino": 0, "conv_impl": 0}),
    ("wino=0,conv_impl=1", {"wino": 0, "conv_impl": 1}),
    ("wino=0,splitk=1,splitk_fused=1", {"wino": 0, "splitk": 1, "splitk_fused": 1}),
    ("wino=0,splitk=1,splitk_fused=0", {"wino": 0, "splitk": 1, "splitk_fused": 0}),
    ("wino_w=0", {"wino_w": 0}),
    ("fuse_head=0", {"fuse_head": 0}),
    ("fuse_first=0", {"fuse_first": 0}),
    ("precision=1", {"precision": 1}),
    ("precision=2", {"precision": 2}),
    ("precision=2,fuse_head=0", {"precision": 2, "fuse_head": 0}),
]
TRIPLES = list(itertools.product((1, 2, 5), (1, 2, 32), (1, 3)))   # (B, chunk, lanes)


_NETS = {}


def unet(feats):
    if feats not in _NETS:
        m = og.UNet(1, 1, feats)
        m.load_state_dict(synth.make_unet_state_dict(feats, seed=11, head_scale=3.0, head_bias=-0.5))
        _NETS[feats] = m.to("cuda:0").eval()
    return _NETS[feats]


def configure(m, opts, chunk=32, lanes=0):
    final = dict(DEFAULTS, **opts)
    final["lanes"] = lanes
    if final["precision"] == 2:
        m.set_option("splitk", 0)      # ("splitk" 1 and "precision" 2 exclude each other, whichever is set second)
    m.set_option("precision", final["precision"])
    for k, v in final.items():
        m.set_option(k, v)
    m.set_chunk(chunk)


def area_inside(mask, boxes):
    """features.py:238 / 241-245 in numpy: count of mask > 0, inside the box if given (x1 < 0: no detection, 0)."""
    if boxes is None:
        return (mask > 0).reshape(len(mask), -1).sum(1).astype(np.int32)
    return np.array([0 if b[0] < 0 else int((mk[b[1]:b[3], b[0]:b[2]] > 0).sum()) for mk, b in zip(mask, boxes)], np.int32)


def noise(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape, dtype=np.uint8)


def boxes_for(B, H, W, roll=0):
    """Rows that include `no detection` (x1 < 0), the whole frame, and a 1x1 box."""
    rows = np.array([[-1, -1, -1, -1], [0, 0, W, H], [3, 2, 4, 3], [5, 3, W - 7, H - 4]], np.int32)
    return np.ascontiguousarray(np.roll(np.resize(rows, (max(B, 4), 4)), roll, axis=0)[:B])


def both_values(mask):
    v = np.unique(mask)
    return v.tolist() == [0, 255]


def usync(m):
    return lambda: check(lib().og_unet_sync(m._h), "og_unet_sync")


def ysync(d):
    return lambda: check(lib().og_yolo_sync(d._h), "og_yolo_sync")


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).reshape(-1).view(np.uint8), np.ascontiguousarray(b).reshape(-1).view(np.uint8))


# ── positive control: first test of the module ─────────────────────────────────
def test_a_positive_control_bgr2gray_overrun_is_reported():
    """og_bgr2gray_dev converts B + 1 frames into a buffer the harness was told holds B: exactly H*W dirty bytes at the start
    of the after-guard, nothing else (the guard is 64 KiB: everything stays inside memory this test owns)."""
    T0[0] = time.time()
    m = unet((32, 64))
    B, H, W = 3, 45, 77
    bgr = noise((B + 1, H, W, 3), 1)
    bgr[B] %= 128          # the overrun's gray bytes stay below 128: none of them equals the guard fill 0xA5 by chance
    rc, pay, faults = G.guarded_call(lambda p: lib().og_bgr2gray_dev(m._h, p["bgr"], B + 1, H, W, p["gray"]), {"bgr": bgr},
                                     {"gray": B * H * W}, "device", usync(m))
    assert rc == 0
    print(f"buffer extents: positive control: {faults}")
    assert [f.key() for f in faults] == [("guard-after", "gray", 0, H * W - 1, H * W)], faults
    from openglottal_amd.utils import bgr_to_gray_numpy

    assert same(pay["gray"], bgr_to_gray_numpy(bgr[:B]))


# ── U-Net chain ────────────────────────────────────────────────────────────────
def _segment(m, entry, label, gray, boxes, want, ref):
    B, H, W = gray.shape
    outs = {"mask": B * H * W if "mask" in want else None, "area": 4 * B if "area" in want else None,
            "logits": 4 * B * H * W if "logits" in want else None}
    fn = getattr(lib(), entry)
    dev = entry.endswith("_dev")
    out = G.run_guarded(entry, f"{label} want={'+'.join(want)}",
                        lambda p: fn(m._h, p["gray"], B, H, W, 0.5, p["boxes"], p["mask"], p["area"], p["logits"]),
                        {"gray": gray, "boxes": boxes}, outs, "device" if dev else "host", usync(m) if dev else None)
    for k in want:
        assert same(out[k], ref[k]), (entry, label, want, k)       # == the Python wrapper on plain buffers
    return out


CHAIN = [((32, 64), 36, 52), ((32, 64), 96, 160), ((33, 66), 32, 64), ((6, 12, 24), 48, 32), (FULL, 64, 48)]


@pytest.mark.parametrize("net", range(len(CHAIN)), ids=[f"{'-'.join(map(str, f))}@{h}x{w}" for f, h, w in CHAIN])
def test_unet_chain(net):
    feats, H, W = CHAIN[net]
    m = unet(feats)
    gray = noise((5, H, W), 100 + net)
    try:
        for oi, (oname, opts) in enumerate(OPTION_SETS):
            k = net * len(OPTION_SETS) + oi
            for ti, (B, chunk, lanes) in enumerate(TRIPLES):
                configure(m, opts, chunk, lanes)
                bx = boxes_for(B, H, W, k + ti) if (k + ti) % 2 else None
                label = f"{feats} {oname} {H}x{W} B={B} chunk={chunk} lanes={lanes} boxes={'given' if bx is not None else 'NULL'}"
                mk, ar, lg = m.segment(gray[:B], boxes=bx, want_logits=True)
                ref = {"mask": mk, "area": ar, "logits": lg}
                assert both_values(mk), label
                for entry in ("og_unet_segment_u8_dev", "og_unet_segment_u8"):
                    _segment(m, entry, label, gray[:B], bx, ("mask", "area", "logits"), ref)
                    if ti % 6 == oi % 6:      # area == NULL switches the fused head's count path; a NULL output changes nothing in the others
                        _segment(m, entry, label, gray[:B], bx, ("mask",), ref)
                        _segment(m, entry, label, gray[:B], bx, ("area",), ref)
                        _segment(m, entry, label, gray[:B], bx, ("mask", "area"), ref)
    finally:
        configure(m, {})


def test_unet_chain_full_256_and_a_70_frame_call():
    """FULL at 256x256, B in {1, 3}: the wave-split / position-split forms and the count slots of the fused head.  70 frames of
    36x52 with chunk 32: two full micro-batches and a ragged one of 6."""
    m = unet(FULL)
    gray = noise((3, 256, 256), 7)
    try:
        for oi, (oname, opts) in enumerate(OPTION_SETS):
            for B in (1, 3):
                configure(m, opts, 32, 0)
                bx = boxes_for(B, 256, 256, oi) if (oi + B) % 2 else None
                label = f"FULL {oname} 256x256 B={B} boxes={'given' if bx is not None else 'NULL'}"
                mk, ar, lg = m.segment(gray[:B], boxes=bx, want_logits=True)
                ref = {"mask": mk, "area": ar, "logits": lg}
                assert both_values(mk), label
                for entry in ("og_unet_segment_u8_dev", "og_unet_segment_u8"):
                    _segment(m, entry, label, gray[:B], bx, ("mask", "area", "logits"), ref)
                    _segment(m, entry, label, gray[:B], bx, ("mask",) if oi % 2 else ("area",), ref)
    finally:
        configure(m, {})
    s = unet((32, 64))
    g70 = noise((70, 36, 52), 8)
    for lanes in (1, 3):
        configure(s, {}, 32, lanes)
        bx = boxes_for(70, 36, 52, lanes)
        mk, ar, lg = s.segment(g70, boxes=bx, want_logits=True)
        for entry in ("og_unet_segment_u8_dev", "og_unet_segment_u8"):
            _segment(s, entry, f"(32, 64) default 36x52 B=70 chunk=32 lanes={lanes}", g70, bx, ("mask", "area", "logits"),
                     {"mask": mk, "area": ar, "logits": lg})
    configure(s, {})


# ── resized path ──────────────────────────────────────────────────────────────
@pytest.mark.parametrize("precision", [0, 2])
def test_resized_path(precision):
    m = unet((32, 64))
    configure(m, {"precision": precision})
    try:
        for (H, W), ch, (nh, nw), B, with_boxes in itertools.product(((45, 77), (131, 67), (1, 300)), (1, 3), ((32, 48), (64, 64)), (1, 3),
                                                                     (False, True)):
            src = noise((B, H, W, ch) if ch == 3 else (B, H, W), H * W + ch)
            bx = boxes_for(B, H, W, B + ch) if with_boxes else None
            if H == 1 and bx is not None:
                bx = np.array([[-1, -1, -1, -1], [0, 0, W, 1], [3, 0, 4, 1]], np.int32)[:B][::-1].copy()
            label = f"precision={precision} {H}x{W}x{ch} -> {nh}x{nw} B={B} boxes={'given' if with_boxes else 'NULL'}"
            mk, ar = m.segment_resized(src, net=(nh, nw), boxes=bx)
            hw, hwn = B * H * W, B * nh * nw
            dev = lambda p: lib().og_unet_segment_resized_u8_dev(m._h, p["src"], B, H, W, ch, nh, nw, 0.5, p["boxes"], p["mask"], p["area"],
                                                                 p["net_logits"], p["net_prob"], p["prob"])
            out = G.run_guarded("og_unet_segment_resized_u8_dev", label, dev, {"src": src, "boxes": bx},
                                {"mask": hw, "area": 4 * B, "net_logits": 4 * hwn, "net_prob": 4 * hwn, "prob": 4 * hw}, "device", usync(m))
            assert same(out["mask"], mk) and same(out["area"], ar), label
            prob, logit = out["prob"].view(np.float32), out["net_logits"].view(np.float32)
            assert same(out["mask"], np.where(prob > 0.5, 255, 0).astype(np.uint8)) and prob.min() < 0.5 < prob.max(), label
            assert logit.min() < 0 < logit.max(), label
            # NULL optional outputs change nothing in the others
            lean = G.run_guarded("og_unet_segment_resized_u8_dev", label + " debug outputs NULL", dev, {"src": src, "boxes": bx},
                                 {"mask": hw, "area": 4 * B, "net_logits": None, "net_prob": None, "prob": None}, "device", usync(m))
            assert same(lean["mask"], mk) and same(lean["area"], ar), label
            only = G.run_guarded("og_unet_segment_resized_u8_dev", label + " mask NULL", dev, {"src": src, "boxes": bx},
                                 {"mask": None, "area": 4 * B, "net_logits": None, "net_prob": None, "prob": 4 * hw}, "device", usync(m))
            assert same(only["area"], ar) and same(only["prob"], out["prob"]), label
            host = G.run_guarded("og_unet_stream_resized_u8", label,
                                 lambda p: lib().og_unet_stream_resized_u8(m._h, p["src"], B, H, W, ch, nh, nw, 0.5, p["boxes"], p["mask"], p["area"]),
                                 {"src": src, "boxes": bx}, {"mask": hw, "area": 4 * B})
            assert same(host["mask"], mk) and same(host["area"], ar), label

            def frames_call(p):
                ptrs = (C.c_void_p * B)(*[p[f"frame{i}"] for i in range(B)])
                return lib().og_unet_stream_frames_resized_u8(m._h, ptrs, B, H, W, ch, nh, nw, 0.5, p["boxes"], p["mask"], p["area"])
            lst = G.run_guarded("og_unet_stream_frames_resized_u8", label, frames_call,
                                dict({f"frame{i}": src[i] for i in range(B)}, boxes=bx), {"mask": hw, "area": 4 * B})
            assert same(lst["mask"], mk) and same(lst["area"], ar), label
    finally:
        configure(m, {})


# ── pipeline kernels ──────────────────────────────────────────────────────────
def test_mask_area_and_stats():
    m = unet((32, 64))
    rs = np.random.RandomState(3)
    for (H, W), B, with_boxes in itertools.product(((63, 65), (64, 64), (17, 241), (45, 77)), (1, 9), (False, True)):
        pred = (rs.rand(B, H, W) > 0.6).astype(np.uint8) * 255
        gt = (rs.rand(B, H, W) > 0.7).astype(np.uint8) * 255
        bx = boxes_for(B, H, W, B + H) if with_boxes else None
        label = f"{H}x{W} B={B} boxes={'given' if with_boxes else 'NULL'}"
        gated = pred.copy()
        if bx is not None:
            gated[:] = 0
            for i, (x1, y1, x2, y2) in enumerate(bx):
                if x1 >= 0:
                    gated[i, y1:y2, x1:x2] = pred[i, y1:y2, x1:x2]
        out = G.run_guarded("og_mask_area_dev", label, lambda p: lib().og_mask_area_dev(m._h, p["mask"], B, H, W, p["boxes"], p["area"]),
                            {"mask": pred, "boxes": bx}, {"area": 4 * B}, "device", usync(m))
        assert out["area"].view(np.int32).tolist() == (gated > 0).reshape(B, -1).sum(1).tolist(), label
        out = G.run_guarded("og_mask_stats_dev", label,
                            lambda p: lib().og_mask_stats_dev(m._h, p["pred"], p["gt"], B, H, W, p["boxes"], p["stats"]),
                            {"pred": pred, "gt": gt, "boxes": bx}, {"stats": 12 * B}, "device", usync(m))
        want = [[int(((gated[i] > 0) & (gt[i] > 0)).sum()), int((gated[i] > 0).sum()), int((gt[i] > 0).sum())] for i in range(B)]
        assert out["stats"].view(np.int32).reshape(B, 3).tolist() == want, label


def test_bgr2gray_dev():
    from openglottal_amd.utils import bgr_to_gray_numpy

    m = unet((32, 64))
    for B, H, W in ((3, 45, 77), (1, 1, 1), (2, 16, 16), (1, 17, 241)):      # n = B*H*W: 10395, 1, 512 (a multiple of 256), 4097
        bgr = noise((B, H, W, 3), B + H)
        out = G.run_guarded("og_bgr2gray_dev", f"{B}x{H}x{W}", lambda p: lib().og_bgr2gray_dev(m._h, p["bgr"], B, H, W, p["gray"]),
                            {"bgr": bgr}, {"gray": B * H * W}, "device", usync(m))
        assert same(out["gray"], bgr_to_gray_numpy(bgr))


def test_canvas_letterbox():
    from openglottal_amd.geometry import letterbox, letterbox_geometry

    m = unet((32, 64))
    sizes = [(256, 256), (256, 512), (128, 512), (208, 352), (512, 256), (512, 128), (352, 208), (301, 217), (17, 400), (255, 257), (1, 1),
             (600, 600), (256, 255), (3, 2), (1024, 768)]        # test_device_canvas_letterbox_equals_host_geometry's
    size, B = 64, len(sizes)
    for ch, value in ((1, 0), (1, 7), (3, 0), (3, 200)):
        frames = [noise(s + ((3,) if ch == 3 else ()), 11 * i + ch) for i, s in enumerate(sizes)]
        gaps = [97 + 13 * i for i in range(B)]     # the offsets are the caller's: slack between the packed frames too
        offsets = np.cumsum([0] + [f.size + g for f, g in zip(frames, gaps)][:-1]).astype(np.int64)
        shapes = np.array(sizes, np.int32)
        geom = np.array([letterbox_geometry(h, w, size) for h, w in sizes], np.int32)

        def packed(fill):
            buf = np.full(int(offsets[-1]) + frames[-1].size, fill, np.uint8)
            for f, o in zip(frames, offsets):
                buf[o:o + f.size] = f.ravel()
            return buf
        want = np.stack([letterbox(f, size, value) for f in frames])
        for entry, kind in (("og_canvas_letterbox_u8_dev", "device"), ("og_canvas_letterbox_u8", "host")):
            fn = getattr(lib(), entry)
            out = G.run_guarded(entry, f"channels={ch} value={value} size={size} B={B} mixed sizes",
                                lambda p: fn(m._h, p["packed"], p["offsets"], p["shapes"], B, ch, size, p["geom"], value, p["out"]),
                                {"packed": packed, "offsets": offsets, "shapes": shapes, "geom": geom}, {"out": B * size * size * ch},
                                kind, usync(m) if kind == "device" else None)
            assert same(out["out"], want), (entry, ch, value)


def _crop_geom(box, size):
    x1, y1, x2, y2 = box
    h, w = y2 - y1, x2 - x1
    scale = size / max(h, w)
    nh, nw = int(round(h * scale)), int(round(w * scale))
    return ((size - nh) // 2, (size - nw) // 2, nh, nw)


def test_segment_crops():
    m = unet((32, 64))
    configure(m, {})
    H, W, size = 96, 160, 32
    good = [(0, 0, W, H), (80, 40, 81, 41), (W - 50, H - 30, W, H), (-1, -1, -1, -1), (10, 5, 90, 77)]
    B = len(good)
    gray = noise((B, H, W), 21)
    boxes = np.array(good, np.int32)
    geom = np.array([_crop_geom(b, size) if b[0] >= 0 else (0, 0, 0, 0) for b in good], np.int32)
    want = m.segment_crops(gray, [b if b[0] >= 0 else None for b in good], crop_size=size)
    assert both_values(want) and not want[3].any()
    host = G.run_guarded("og_unet_segment_crops_u8", f"{H}x{W} size={size} B={B}",
                         lambda p: lib().og_unet_segment_crops_u8(m._h, p["gray"], B, H, W, p["boxes"], p["geom"], size, 0.5, p["out_masks"]),
                         {"gray": gray, "boxes": boxes, "geom": geom}, {"out_masks": B * H * W})
    assert same(host["out_masks"], want)
    # the device variant also gets a record that reaches outside the frame and a stale geom: zeros, not an out-of-bounds access
    boxes_d = np.concatenate([boxes, [[100, 50, 200, 120], [10, 5, 90, 77]]]).astype(np.int32)
    geom_d = np.concatenate([geom, [list(_crop_geom((100, 50, 200, 120), size)), [0, 0, 40, 32]]]).astype(np.int32)
    gray_d = np.concatenate([gray, noise((2, H, W), 22)])
    Bd = B + 2
    dev = G.run_guarded("og_unet_segment_crops_u8_dev", f"{H}x{W} size={size} B={Bd} (one out-of-frame box, one stale geom)",
                        lambda p: lib().og_unet_segment_crops_u8_dev(m._h, p["gray"], Bd, H, W, p["boxes"], p["geom"], size, 0.5, p["tiles"],
                                                                     p["tile_masks"], p["out_masks"]),
                        {"gray": gray_d, "boxes": boxes_d, "geom": geom_d},
                        {"tiles": Bd * size * size, "tile_masks": Bd * size * size, "out_masks": Bd * H * W}, "device", usync(m))
    got = dev["out_masks"].reshape(Bd, H, W)
    assert same(got[:B], want) and not got[B:].any() and not dev["tiles"].reshape(Bd, -1)[B:].any()


# ── detector ────────────────────────────────────────────────────────────────
_DETS = {}


def detector(precision):
    from openglottal_amd.yolo import YoloV8Detector

    if precision not in _DETS:
        _DETS[precision] = YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0", precision=precision)
    return _DETS[precision]


def yconfigure(d, **opts):
    for k, v in dict({"latency_batch": 1, "head_fused": 1, "zero_copy": 1, "source_stage_kib": 65536, "source_mapped": 1}, **opts).items():
        d.set_option(k, v)


def _detect(d, entry, label, frames, want_pred, ref_best, ref_pred):
    B, H, W = frames.shape[:3]
    A = lib().og_yolo_num_anchors(d._h, H, W)
    fn = getattr(lib(), entry)
    dev = entry.endswith("_dev")
    out = G.run_guarded(entry, f"{label} pred={'given' if want_pred else 'NULL'}",
                        lambda p: fn(d._h, p["bgr"], B, H, W, CONF, p["best"], p["pred"]), {"bgr": frames},
                        {"best": 20 * B, "pred": 20 * B * A if want_pred else None}, "device" if dev else "host", ysync(d) if dev else None)
    assert same(out["best"], ref_best), (entry, label)
    if want_pred:
        assert same(out["pred"], ref_pred), (entry, label)


@pytest.mark.parametrize("precision", ["f32", "f16"])
@pytest.mark.parametrize("shape", [(32, 32), (96, 160), (256, 256)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_detector(shape, precision):
    """32x32: 21 anchors, 96x160: 315 (neither a multiple of 64), 256x256: 1344."""
    d = detector(precision)
    H, W = shape
    assert lib().og_yolo_num_anchors(d._h, H, W) == {32: 21, 96: 315, 256: 1344}[H]
    frames = noise((70, H, W, 3), H + W)
    hits = 0
    try:
        for lb, hf, B in itertools.product((0, 1, 3), (0, 1), (1, 3, 70)):
            yconfigure(d, latency_batch=lb, head_fused=hf)
            best, pred = d.detect_batch(frames[:B], CONF, want_pred=True)
            hits += int((best[:, 4] >= 0).sum())
            label = f"{precision} {H}x{W} B={B} latency_batch={lb} head_fused={hf}"
            for entry in ("og_yolo_detect_u8_dev", "og_yolo_detect_u8"):
                for want_pred in (False, True):
                    _detect(d, entry, label, frames[:B], want_pred, best, pred)
    finally:
        yconfigure(d)
    assert hits > 0, "no detector row was a detection: the matrix compared `no detection` rows only"


def test_detector_zero_copy_and_begin_end():
    from openglottal_amd.yolo import letterbox_bgr  # noqa: F401  (the resized begin letterboxes on the device)

    hits = 0
    for precision in ("f32", "f16"):
        d = detector(precision)
        frames = noise((3, 96, 160, 3), 31)
        odd = noise((3, 100, 120, 3), 32)
        try:
            per_zc = []
            for zc in (0, 1):
                yconfigure(d, zero_copy=zc)
                got = []
                for B in (1, 3):
                    best = d.detect_batch(frames[:B], CONF)
                    hits += int((best[:, 4] >= 0).sum())
                    label = f"{precision} 96x160 B={B} zero_copy={zc}"
                    _detect(d, "og_yolo_detect_u8", label, frames[:B], False, best, None)

                    def begin_end(p):
                        rc = lib().og_yolo_detect_u8_begin(d._h, p["bgr"], B, 96, 160, CONF)
                        return rc or lib().og_yolo_detect_u8_end(d._h, p["best"])
                    out = G.run_guarded("og_yolo_detect_u8_begin", label, begin_end, {"bgr": frames[:B]}, {"best": 20 * B})
                    G.CASES["og_yolo_detect_u8_end"] += 1
                    assert same(out["best"], best), label
                    ref = d.detect_frames(odd[:B], CONF)

                    def rbegin_end(p):
                        rc = lib().og_yolo_detect_resized_u8_begin(d._h, p["src"], B, 100, 120, 3, 256, CONF)
                        return rc or lib().og_yolo_detect_u8_end(d._h, p["best"])
                    out = G.run_guarded("og_yolo_detect_resized_u8_begin", label.replace("96x160", "100x120"), rbegin_end, {"src": odd[:B]},
                                        {"best": 20 * B})
                    G.CASES["og_yolo_detect_u8_end"] += 1
                    assert same(out["best"], ref), label
                    got.append((best, ref))
                per_zc.append(got)
            for (a, ra), (b, rb) in zip(*per_zc):      # the two zero_copy settings agree bit for bit
                assert same(a, b) and same(ra, rb), precision
        finally:
            yconfigure(d)
    assert hits > 0


@pytest.mark.parametrize("ch", [1, 3])
def test_yolo_letterbox_dev(ch):
    from openglottal_amd.yolo import letterbox_bgr

    d = detector("f32")
    for (H, W), B in itertools.product(((33, 70), (100, 120), (299, 500), (224, 256)), (1, 3)):
        src = noise((B, H, W, 3) if ch == 3 else (B, H, W), H + W + ch)
        want = np.stack([letterbox_bgr(f if ch == 3 else np.repeat(f[..., None], 3, axis=-1), 256)[0] for f in src])
        out = G.run_guarded("og_yolo_letterbox_u8_dev", f"{H}x{W}x{ch} B={B}",
                            lambda p: lib().og_yolo_letterbox_u8_dev(d._h, p["src"], B, H, W, ch, 256, p["out"]), {"src": src},
                            {"out": want.size}, "device", ysync(d))
        assert same(out["out"], want), (H, W, ch, B)


@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_detector_resized(precision):
    """100x120 and 33x700 (12 content rows between two pads of 114)."""
    d = detector(precision)
    hits = {}
    try:
        for (H, W), kib, mapped, B in itertools.product(((100, 120), (33, 700)), (65536, 1), (0, 1), (1, 3, 70)):
            yconfigure(d, source_stage_kib=kib, source_mapped=mapped)       # (1 KiB: below one frame, every frame is staged alone)
            ch = 3 if (B + mapped) % 2 else 1
            src = noise((B, H, W, 3) if ch == 3 else (B, H, W), H + W)
            ref = d.detect_frames(src, CONF)
            hits[(H, W)] = hits.get((H, W), 0) + int((ref[:, 4] >= 0).sum())
            label = f"{precision} {H}x{W}x{ch} B={B} source_stage_kib={kib} source_mapped={mapped}"
            out = G.run_guarded("og_yolo_detect_resized_u8_dev", label,
                                lambda p: lib().og_yolo_detect_resized_u8_dev(d._h, p["src"], B, H, W, ch, 256, CONF, p["best"]), {"src": src},
                                {"best": 20 * B}, "device", ysync(d))
            assert same(out["best"], ref), label
            out = G.run_guarded("og_yolo_detect_resized_u8", label,
                                lambda p: lib().og_yolo_detect_resized_u8(d._h, p["src"], B, H, W, ch, 256, CONF, p["best"]), {"src": src},
                                {"best": 20 * B})
            assert same(out["best"], ref), label
    finally:
        yconfigure(d)
    print(f"buffer extents: detector rows with a detection per shape ({precision}): {hits}")
    assert hits[(100, 120)] > 0 and hits[(33, 700)] > 0


# ── host streaming and zero copy ────────────────────────────────────────────────
@pytest.mark.parametrize("net", ["FULL@256x256", "32-64@96x160"])
def test_host_streaming_and_zero_copy(net):
    """`zero_copy` in {0, 1} x `fuse_head` in {0, 1}: with the unfused head k_head adds its counts into the host-mapped `area`
    with atomicAdd.  The two zero_copy settings must agree bit for bit."""
    feats, H, W = (FULL, 256, 256) if net.startswith("FULL") else ((32, 64), 96, 160)
    m = unet(feats)
    bgr = noise((5, H, W, 3), 41)
    from openglottal_amd.utils import bgr_to_gray

    gray = bgr_to_gray(bgr)
    try:
        for fh in (1, 0):
            configure(m, {"fuse_head": fh})
            ref_mask, ref_area, _ = m.segment(gray)      # (5 frames: the copy path)
            assert both_values(ref_mask) and same(ref_area, area_inside(ref_mask, None))
            for ch, B, with_boxes in itertools.product((1, 3), (1, 3, 4, 5), (False, True)):
                frames = bgr[:B] if ch == 3 else gray[:B]
                bx = boxes_for(B, H, W, B) if with_boxes else None
                want_area = area_inside(ref_mask[:B], bx)
                got = []
                for zc in (0, 1):
                    m.set_option("zero_copy", zc)
                    label = f"{feats} {H}x{W}x{ch} B={B} zero_copy={zc} fuse_head={fh} boxes={'given' if with_boxes else 'NULL'}"
                    call = lambda p: lib().og_unet_stream_u8(m._h, p["frames"], B, H, W, ch, 0.5, p["boxes"], p["mask"], p["area"])
                    for source in ("pageable", "pinned"):
                        out = G.run_guarded("og_unet_stream_u8", f"{label} source={source}", call, {"frames": frames, "boxes": bx},
                                            {"mask": B * H * W, "area": 4 * B}, input_kinds={"frames": "pinned"} if source == "pinned" else None)
                        assert same(out["mask"], ref_mask[:B]) and same(out["area"], want_area), (label, source, out["area"].view(np.int32), want_area)
                        got.append(out)
                    out = G.run_guarded("og_unet_stream_u8", f"{label} source=pinned mask=NULL", call, {"frames": frames, "boxes": bx},
                                        {"mask": None, "area": 4 * B}, input_kinds={"frames": "pinned"})
                    assert same(out["area"], want_area), label

                    def frames_call(p):
                        ptrs = (C.c_void_p * B)(*[p[f"frame{i}"] for i in range(B)])
                        return lib().og_unet_stream_frames_u8(m._h, ptrs, B, H, W, ch, 0.5, p["boxes"], p["mask"], p["area"])
                    out = G.run_guarded("og_unet_stream_frames_u8", label, frames_call, dict({f"frame{i}": frames[i] for i in range(B)}, boxes=bx),
                                        {"mask": B * H * W, "area": 4 * B})
                    assert same(out["mask"], ref_mask[:B]) and same(out["area"], want_area), label
                    got.append(out)
                for o in got[1:]:
                    assert same(o["mask"], got[0]["mask"]) and same(o["area"], got[0]["area"])
    finally:
        configure(m, {})


# ── parity entries ──────────────────────────────────────────────────────────
def test_parity_entries():
    m = unet((32, 64))
    configure(m, {})
    B, H, W = 2, 36, 52
    x = np.random.RandomState(5).rand(B, 1, H, W).astype(np.float32)
    want = m(x)
    out = G.run_guarded("og_unet_forward_f32", f"(32, 64) {H}x{W} B={B}",
                        lambda p: lib().og_unet_forward_f32(m._h, p["x"], B, H, W, p["logits"]), {"x": x}, {"logits": 4 * B * H * W})
    assert same(out["logits"], want) and want.min() < 0 < want.max()
    for name, (c, h, w) in (("downs.0.b", (32, H, W)), ("pool1", (64, H // 4, W // 4)), ("ups.3.b", (32, H, W))):
        n = B * c * h * w
        dims = (C.c_int * 3)()
        out = G.run_guarded("og_unet_get_activation", f"{name} capacity = B*C*H*W",
                            lambda p: lib().og_unet_get_activation(m._h, name.encode(), B, p["out"], n, dims), {}, {"out": 4 * n})
        assert tuple(dims) == (c, h, w) and same(out["out"], m.activation(name, B))
        rc, pay, faults = G.guarded_call(lambda p: lib().og_unet_get_activation(m._h, name.encode(), B, p["out"], n - 1, dims), {}, {"out": 4 * n})
        assert rc == OG_EINVAL and not faults and np.all(pay["out"] == G.GUARD_FILL), name    # refused: payload and guards untouched
    d = detector("f32")
    yconfigure(d)
    d.detect_batch(noise((2, 96, 160, 3), 6), CONF)
    for name in ("model.0", "model.21", "cls2"):
        ref = d.activation(name, 2)
        n = ref.size
        dims = (C.c_int * 3)()
        out = G.run_guarded("og_yolo_get_activation", f"{name} capacity = B*C*H*W",
                            lambda p: lib().og_yolo_get_activation(d._h, name.encode(), 2, p["out"], n, dims), {}, {"out": 4 * n})
        assert tuple(dims) == ref.shape[1:] and same(out["out"], ref)
        rc, pay, faults = G.guarded_call(lambda p: lib().og_yolo_get_activation(d._h, name.encode(), 2, p["out"], n - 1, dims), {}, {"out": 4 * n})
        assert rc == OG_EINVAL and not faults and np.all(pay["out"] == G.GUARD_FILL), name


# ── alignment ────────────────────────────────────────────────────────────────
def test_misaligned_pointers_are_refused_before_anything_runs():
    """The header's rule: int32 / float buffers 4-byte aligned, `offsets` (int64) and `frame_ptrs` 8-byte aligned, u8 buffers
    any address.  Each call below has ONE pointer off its alignment and must return OG_EINVAL with every buffer untouched;
    nothing is launched on a misaligned pointer."""
    import torch

    m, d = unet((32, 64)), detector("f32")
    configure(m, {})
    yconfigure(d)
    B, H, W = 2, 36, 52
    dev = torch.full((1 << 20,), G.GUARD_FILL, dtype=torch.uint8, device="cuda:0")
    host = np.full(1 << 20, G.GUARD_FILL, np.uint8)
    torch.cuda.synchronize()
    l, uh, yh = lib(), m._h, d._h
    n = 0
    for base in (dev.data_ptr(), host.ctypes.data):
        on_dev = base == dev.data_ptr()
        a = [base + (i << 16) for i in range(12)]      # twelve aligned 64 KiB buffers

        def variants(idx, offs=(1, 2)):
            """Argument lists with exactly one of the pointers `idx` moved off its alignment."""
            for i in idx:
                for o in offs:
                    v = list(a)
                    v[i] += o
                    yield v
        calls = []
        if on_dev:
            for v in variants((1, 3, 4)):
                calls.append(l.og_unet_segment_u8_dev(uh, v[0], B, H, W, 0.5, v[1], v[2], v[3], v[4]))
            for v in variants((1, 3, 4, 5, 6)):
                calls.append(l.og_unet_segment_resized_u8_dev(uh, v[0], B, 45, 77, 1, 32, 48, 0.5, v[1], v[2], v[3], v[4], v[5], v[6]))
            for v in variants((1, 2)):
                calls.append(l.og_mask_area_dev(uh, v[0], B, H, W, v[1], v[2]))
            for v in variants((2, 3)):
                calls.append(l.og_mask_stats_dev(uh, v[0], v[1], B, H, W, v[2], v[3]))
            for v in variants((1,), (1, 2, 4)):
                calls.append(l.og_canvas_letterbox_u8_dev(uh, v[0], v[1], v[2], 1, 1, 64, v[3], 0, v[4]))
            for v in variants((2, 3)):
                calls.append(l.og_canvas_letterbox_u8_dev(uh, v[0], v[1], v[2], 1, 1, 64, v[3], 0, v[4]))
            for v in variants((1, 2)):
                calls.append(l.og_unet_segment_crops_u8_dev(uh, v[0], B, 96, 160, v[1], v[2], 32, 0.5, v[3], v[4], v[5]))
            for v in variants((1, 2)):
                calls.append(l.og_yolo_detect_u8_dev(yh, v[0], 1, 32, 32, CONF, v[1], v[2]))
            for v in variants((1,)):
                calls.append(l.og_yolo_detect_resized_u8_dev(yh, v[0], 1, 33, 70, 3, 256, CONF, v[1]))
        else:
            for v in variants((1, 3, 4)):
                calls.append(l.og_unet_segment_u8(uh, v[0], B, H, W, 0.5, v[1], v[2], v[3], v[4]))
            for v in variants((1, 3)):
                calls.append(l.og_unet_stream_u8(uh, v[0], B, H, W, 1, 0.5, v[1], v[2], v[3]))
                calls.append(l.og_unet_stream_resized_u8(uh, v[0], B, 45, 77, 1, 32, 48, 0.5, v[1], v[2], v[3]))
            for v in variants((0,), (1, 2, 4)):
                calls.append(l.og_unet_stream_frames_u8(uh, v[0], B, H, W, 1, 0.5, v[1], v[2], v[3]))
                calls.append(l.og_unet_stream_frames_resized_u8(uh, v[0], B, 45, 77, 1, 32, 48, 0.5, v[1], v[2], v[3]))
            for v in variants((0, 1)):
                calls.append(l.og_unet_forward_f32(uh, v[0], 1, H, W, v[1]))
            for v in variants((1,), (1, 2, 4)):
                calls.append(l.og_canvas_letterbox_u8(uh, v[0], v[1], v[2], 1, 1, 64, v[3], 0, v[4]))
            for v in variants((1, 2)):
                calls.append(l.og_unet_segment_crops_u8(uh, v[0], B, 96, 160, v[1], v[2], 32, 0.5, v[3]))
                calls.append(l.og_yolo_detect_u8(yh, v[0], 1, 32, 32, CONF, v[1], v[2]))
            for v in variants((1,)):
                calls.append(l.og_yolo_detect_resized_u8(yh, v[0], 1, 33, 70, 3, 256, CONF, v[1]))
            m.segment(noise((1, H, W), 1))
            dims = (C.c_int * 3)()
            calls.append(l.og_unet_get_activation(uh, b"downs.0.b", 1, a[0] + 2, 1 << 14, dims))
        assert calls and all(rc == OG_EINVAL for rc in calls), calls
        n += len(calls)
    check(l.og_unet_sync(uh), "og_unet_sync")
    check(l.og_yolo_sync(yh), "og_yolo_sync")
    assert bool((dev == G.GUARD_FILL).all()) and bool((host == G.GUARD_FILL).all())      # no refused call touched a buffer
    # a begin / end pair: the misaligned `best` is refused with the call still in flight, the aligned one then delivers it
    fr = noise((1, 32, 32, 3), 2)
    assert l.og_yolo_detect_u8_begin(yh, fr.ctypes.data, 1, 32, 32, CONF) == 0
    best = np.empty(8, np.float32)
    assert l.og_yolo_detect_u8_end(yh, best.ctypes.data + 2) == OG_EINVAL
    assert l.og_yolo_detect_u8_end(yh, best.ctypes.data) == 0 and same(best[:5], d.detect_batch(fr, CONF)[0])
    print(f"buffer extents: {n + 1} misaligned calls refused")


# ── report: last test of the module ────────────────────────────────────────────
def test_z_report_cases_per_entry_point(request):
    print(G.report())
    ran = {i.name.split("[")[0] for i in request.session.items if i.fspath == request.node.fspath}      # (a -k run selects fewer)
    missing = [e for e, tests in MATRIX.items() if set(tests.split()) <= ran and not G.CASES[e]]
    assert not missing, f"entries of the matrix that no case of this run called inside guards: {missing}"
    if T0[0]:
        print(f"buffer extents: module wall time {time.time() - T0[0]:.1f} s")
