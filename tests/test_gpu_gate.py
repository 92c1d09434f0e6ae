"""-m gpu: the U-Net on the kept frames only (include/openglottal_hip_gate.h): k_gate_select against its host twin,
k_gate_gather / k_gate_scatter against numpy indexing inside guard zones, og_gated_segment_kept_dev with SCRIPTED boxes against
og_unet_segment_resized_u8_dev on every frame, the stream entries against og_gated_stream_u8 run in the same test, and the Python
layers on top.  Everything is compared bit for bit: a frame's mask and area are a function of the frame alone.

Nets and frames follow tests/test_gpu_gated.py (the recipe is copied): widths (4, 8, 16, 32), N = 70."""
import numpy as np
import pytest

import gate_cases as GC
import openglottal_amd as og
from openglottal_amd import features, gated, infer as I, synth
from openglottal_amd._lib import check, lib
from openglottal_amd.yolo import YoloV8Detector

pytestmark = pytest.mark.gpu

N = 70
FEATS = (4, 8, 16, 32)
CASES = {                       # name -> (H, W, channels, precision)
    "bgr-256x256": (256, 256, 3, "f32"),        # the letterbox is the identity, the U-Net runs its plain chain
    "bgr-96x160": (96, 160, 3, "f32"),
    "gray-100x120": (100, 120, 1, "f32"),
    "bgr-96x160-f16": (96, 160, 3, "f16"),      # both networks at "precision" 2
}
_NETS, _FR = {}, {}


def nets(precision):
    if precision not in _NETS:
        m = og.UNet(1, 1, FEATS)
        m.load_state_dict(synth.make_unet_state_dict(FEATS, seed=5, head_scale=3.0, head_bias=0.0))
        m.to("cuda:0").eval()
        if precision == "f16":
            m.set_option("precision", 2)
        d = YoloV8Detector(synth.make_yolov8_state_dict(seed=7), device="cuda:0", precision=precision)
        _NETS[precision] = (m, d, gated.GatedEngine(m, d))
    return _NETS[precision]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


def frames_of(name):
    """The case's frames and the detector's raw confidences on them, computed once."""
    if name not in _FR:
        H, W, ch, precision = CASES[name]
        rs = np.random.RandomState(H * 1000 + W + ch)
        fr = rs.randint(0, 256, (N, H, W, 3) if ch == 3 else (N, H, W), dtype=np.uint8)
        raw = nets(precision)[1].detect_frames(fr, 0.0)[:, 4]
        _FR[name] = (fr, raw)
    return _FR[name]


def det_state(det):
    return (det._centre, det._size, det._misses)


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ── the three kernels ─────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("B", GC.SELECT_B)
def test_k_gate_select_equals_the_host_twin(B):
    import torch

    e = nets("f32")[2]
    for name, kept in GC.patterns(B).items():
        boxes = GC.boxes_for(kept)
        want = gated.select_host(boxes)
        assert np.array_equal(want, GC.keep_of(boxes)), name
        d_keep = torch.full((B + 8,), -7, dtype=torch.int32, device="cuda:0")
        d_count = torch.full((3,), -7, dtype=torch.int32, device="cuda:0")
        d_boxes = dev(boxes) if B else None
        torch.cuda.synchronize()
        check(lib().og_gate_select_dev(e._h, d_boxes.data_ptr() if B else None, B, d_keep.data_ptr(), d_count[1:].data_ptr()), "og_gate_select_dev")
        e.sync()
        keep, count = d_keep.cpu().numpy(), d_count.cpu().numpy()
        assert count.tolist() == [-7, len(want), -7], (name, count)
        assert np.array_equal(keep[:len(want)], want) and (keep[len(want):] == -7).all(), name      # nothing past the count is written


GUARD = 1 << 16
ROW_BYTES = (4, 16, 20, 4096, 4112, 12000, 29391)      # areas, boxes, odd, a multiple of 16 and one past the next, 100x120, 97x101x3


def _zone(nbytes, off):
    """A device allocation [guard | payload | guard] of 0xA5 whose payload starts `off` bytes past a multiple of 256."""
    import torch

    raw = torch.full((2 * GUARD + nbytes + 512,), 0xA5, dtype=torch.uint8, device="cuda:0")
    lo = GUARD + (-(raw.data_ptr() + GUARD)) % 256 + off
    return raw, lo


@pytest.mark.parametrize("row_bytes", ROW_BYTES)
def test_k_gate_gather_and_scatter_equal_numpy_indexing_inside_guards(row_bytes):
    import torch

    e = nets("f32")[2]
    B = 37
    rs = np.random.RandomState(row_bytes)
    for n in (1, B - 1, B):
        keep = np.sort(rs.choice(B, n, replace=False)).astype(np.int32)
        d_keep = dev(keep)
        for src_off in (0, 1):
            for dst_off in (0, 1):
                label = (row_bytes, n, src_off, dst_off)
                # gather: B source rows -> n dense rows
                rows = rs.randint(1, 256, (B, row_bytes), dtype=np.uint8)
                s_raw, s_lo = _zone(B * row_bytes, src_off)
                s_raw[s_lo:s_lo + B * row_bytes] = dev(rows).reshape(-1)
                d_raw, d_lo = _zone(n * row_bytes, dst_off)
                torch.cuda.synchronize()
                check(lib().og_gate_gather_dev(e._h, s_raw.data_ptr() + s_lo, row_bytes, d_keep.data_ptr(), n, d_raw.data_ptr() + d_lo), "gather")
                e.sync()
                got = d_raw.cpu().numpy()
                assert np.array_equal(got[d_lo:d_lo + n * row_bytes].reshape(n, row_bytes), rows[keep]), label
                assert (got[:d_lo] == 0xA5).all() and (got[d_lo + n * row_bytes:] == 0xA5).all(), label
                # scatter: n dense rows -> B rows, the others zero
                dense = rs.randint(1, 256, (n, row_bytes), dtype=np.uint8)
                s_raw, s_lo = _zone(n * row_bytes, src_off)
                s_raw[s_lo:s_lo + n * row_bytes] = dev(dense).reshape(-1)
                d_raw, d_lo = _zone(B * row_bytes, dst_off)
                torch.cuda.synchronize()
                check(lib().og_gate_scatter_dev(e._h, s_raw.data_ptr() + s_lo, row_bytes, d_keep.data_ptr(), n, B, d_raw.data_ptr() + d_lo), "scatter")
                e.sync()
                got = d_raw.cpu().numpy()
                want = np.zeros((B, row_bytes), np.uint8)
                want[keep] = dense
                assert np.array_equal(got[d_lo:d_lo + B * row_bytes].reshape(B, row_bytes), want), label
                assert (got[:d_lo] == 0xA5).all() and (got[d_lo + B * row_bytes:] == 0xA5).all(), label


# ── the building block, with scripted boxes ───────────────────────────────────────────────────────────────────────────
REGIMES = ("none", "first only", "last only", "all", "alternating")


@pytest.mark.parametrize("name", list(CASES))
def test_segment_kept_dev_equals_the_network_on_every_frame(name):
    import torch

    H, W, ch, precision = CASES[name]
    m, d, e = nets(precision)
    fr, _ = frames_of(name)
    src = dev(fr)
    pats = GC.patterns(N)
    for regime in REGIMES:
        boxes = GC.boxes_for(pats[regime], W, H)
        keep = GC.keep_of(boxes)
        bx = dev(boxes)
        area_ref = torch.full((N,), -3, dtype=torch.int32, device="cuda:0")
        mask_ref = torch.full((N, H, W), 7, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        m.segment_resized_dev(src, N, H, W, ch, 256, 256, area_ref, 0.5, boxes_dev=bx, mask_dev=mask_ref)
        m.sync()
        area_ref, mask_ref = area_ref.cpu().numpy(), mask_ref.cpu().numpy()
        for with_mask in (True, False):
            area = torch.full((N,), -3, dtype=torch.int32, device="cuda:0")
            mask = torch.full((N, H, W), 7, dtype=torch.uint8, device="cuda:0") if with_mask else None
            torch.cuda.synchronize()
            n = e.segment_kept_dev(src, N, H, W, ch, bx, area, mask_dev=mask, threshold=0.5)
            e.sync()
            assert n == len(keep) == len(gated.select_host(boxes)), (regime, n)
            assert same_bits(area.cpu().numpy(), area_ref), (regime, with_mask)
            if with_mask:
                got = mask.cpu().numpy()
                want = np.zeros_like(mask_ref)
                want[keep] = mask_ref[keep]
                assert same_bits(got, want), regime
        if regime == "all":
            assert area_ref.max() > 0 and (mask_ref > 0).any()
    assert same_bits(src.cpu().numpy(), fr)                            # the frames were only read


# ── the stream entries ────────────────────────────────────────────────────────────────────────────────────────────────
def stage_for(e, H, W, ch, frames_per_micro_batch=25):
    kib = -(-frames_per_micro_batch * H * W * ch // 1024)       # rounded up: room for exactly that many frames
    mbs, _ = gated.gate_plan(N, H, W, ch, kib)
    assert [nb for _, nb in mbs] == [25, 25, 20], mbs
    e.set_option("stage_kib", kib)
    return mbs


def _pair(e, src, **kw):
    """The plain engine and the kept mode on the same frames from a reset tracker: (plain, kept, plain state, kept state)."""
    e.reset()
    plain = e.run(src, want_boxes=True, want_best=True, want_mask=True, **kw)
    st_plain = e.get_state().as_tuple()
    e.reset()
    kept = e.run(src, want_boxes=True, want_best=True, want_mask=True, skip_unboxed=True, **kw)
    return plain, kept, st_plain, e.get_state().as_tuple()


def _check_pair(plain, kept, label):
    for k in ("area", "boxes", "best"):
        assert same_bits(kept[k], plain[k]), (label, k)
    boxed = plain["boxes"][:, 0] >= 0
    assert kept["kept"] == int(boxed.sum()), label
    assert same_bits(kept["mask"][boxed], plain["mask"][boxed]), label
    assert not kept["mask"][~boxed].any(), label
    assert not plain["area"][~boxed].any(), label


@pytest.mark.parametrize("as_list", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_the_kept_stream_equals_the_plain_engine_bit_for_bit(name, as_list):
    H, W, ch, precision = CASES[name]
    m, d, e = nets(precision)
    fr, raw = frames_of(name)
    src = list(fr) if as_list else fr
    try:
        mbs = stage_for(e, H, W, ch)
        # every frame kept: any detection is accepted, no jump is a miss -> every micro-batch takes the in-place path
        e.set_params(max_shift_px=1e9)
        plain, kept, s0, s1 = _pair(e, src, conf=0.0)
        assert s0 == s1 and kept["kept"] == N and (plain["boxes"][:, 0] >= 0).all()
        _check_pair(plain, kept, "all kept")
        # no frame kept: no confidence exceeds 2 -> no network call, everything zero
        e.set_params()
        plain, kept, s0, s1 = _pair(e, src, conf=2.0)
        assert s0 == s1 and kept["kept"] == 0 and not kept["area"].any() and not kept["mask"].any()
        _check_pair(plain, kept, "none kept")
        # mixed: about half of the frames have a detection
        plain, kept, s0, s1 = _pair(e, src, conf=float(np.median(raw)))
        assert s0 == s1
        per_mb = [int((kept["boxes"][b0:b0 + nb, 0] >= 0).sum()) for b0, nb in mbs]
        assert any(0 < n < nb for n, (_, nb) in zip(per_mb, mbs)), per_mb       # gather, network on n frames and scatter did run
        assert plain["area"].max() > 0
        _check_pair(plain, kept, "mixed")
        # areas alone, at the default setting (one micro-batch)
        e.set_option("stage_kib", 65536)
        e.reset()
        alone = e.run(src, conf=float(np.median(raw)), want_boxes=False, skip_unboxed=True)
        assert same_bits(alone["area"], plain["area"]) and alone["kept"] == kept["kept"]
    finally:
        e.set_option("stage_kib", 65536)
        e.set_params()


def test_a_second_kept_call_continues_the_tracker_and_reset_restarts_it():
    H, W, ch, _ = CASES["bgr-96x160"]
    m, d, e = nets("f32")
    fr, raw = frames_of("bgr-96x160")
    conf = float(np.median(raw))
    e.set_params()
    e.reset()
    ref = e.run(fr, conf=conf, want_best=True)
    e.reset()
    a = e.run(fr[:41], conf=conf, skip_unboxed=True)
    b = e.run(fr[41:], conf=conf, skip_unboxed=True)
    assert same_bits(np.concatenate([a["boxes"], b["boxes"]]), ref["boxes"]) and same_bits(np.concatenate([a["area"], b["area"]]), ref["area"])
    assert a["kept"] + b["kept"] == int((ref["boxes"][:, 0] >= 0).sum())
    st = e.get_state()                                         # without a reset the tracker goes on: the host twin from that state
    c = e.run(fr[:20], conf=conf, skip_unboxed=True)
    want = gated.track_host(st, gated.params_of(), ref["best"][:20], W, H)
    assert same_bits(c["boxes"], want) and e.get_state().as_tuple() == st.as_tuple()
    e.reset()
    assert same_bits(e.run(fr[:20], conf=conf, skip_unboxed=True)["boxes"], ref["boxes"][:20])
    e.reset()                                                  # resets inside a call
    resets = np.zeros(N, np.uint8)
    resets[::7] = 1
    every = e.run(fr, conf=conf, resets=resets, skip_unboxed=True)
    st0 = gated.TrackState()
    assert same_bits(every["boxes"], gated.track_host(st0, gated.params_of(), ref["best"], W, H, resets))
    e.reset()
    plain = e.run(fr, conf=conf, resets=resets)
    assert same_bits(every["area"], plain["area"]) and same_bits(every["boxes"], plain["boxes"])


# ── Python on top ─────────────────────────────────────────────────────────────────────────────────────────────────────
@pytest.mark.parametrize("name", ["bgr-96x160", "gray-100x120", "bgr-96x160-f16"])
def test_area_waveform_on_the_device_with_skip_unboxed_equals_the_staged_default(name):
    m, d, _ = nets(CASES[name][3])
    fr, raw = frames_of(name)
    conf = float(np.median(raw))
    det0 = og.TemporalDetector(d, conf=conf)
    want = features.area_waveform(fr, det0, m, engine="staged")
    assert want.max() > 0 and (want == 0).any()
    for src in (fr, list(fr)):
        det = og.TemporalDetector(d, conf=conf)
        n0 = gated.GatedEngine.passes
        wave = features.area_waveform(src, det, m, engine="device", skip_unboxed=True)
        assert gated.GatedEngine.passes == n0 + 1
        assert wave.dtype == np.float64 and np.array_equal(wave, want) and det_state(det) == det_state(det0)
    det = og.TemporalDetector(d, conf=conf)                    # the staged pass compacts on the host: the same waveform again
    assert np.array_equal(features.area_waveform(fr, det, m, engine="staged", skip_unboxed=True), want) and det_state(det) == det_state(det0)
    feats = og.extract_gaw_features(fr, 4000.0, og.TemporalDetector(d, conf=conf), m)
    ref = features._kinematic_features([float(v) for v in want])
    assert np.array_equal(feats["_area"], ref["_area"]) and feats["f0"] == (None if ref["f0"] is None else ref["f0"] * 4000.0)


@pytest.mark.parametrize("name", ["bgr-96x160", "bgr-256x256"])
def test_run_pipeline_with_skip_unboxed_equals_the_default_byte_for_byte(name):
    m, d, _ = nets("f32")
    fr, raw = frames_of(name)
    conf = float(np.median(raw))
    for style in ("fill", "none"):
        want = I.run_pipeline(fr, og.TemporalDetector(d, conf=conf), "unet", m, "cuda:0", overlay_style=style)
        got = I.run_pipeline(fr, og.TemporalDetector(d, conf=conf), "unet", m, "cuda:0", overlay_style=style, skip_unboxed=True)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), style
        assert want[1].max() > 0 and (want[1] == 0).any()
    assert not same_bits(I.run_pipeline(fr, og.TemporalDetector(d, conf=conf), "unet", m, "cuda:0", overlay_style="fill")[0],
                         I.run_pipeline(fr, og.TemporalDetector(d, conf=conf), "unet", m, "cuda:0", overlay_style="none")[0])
    with pytest.raises(og.OpenGlottalHipError):
        I.run_pipeline(fr, None, "unet-only", m, "cuda:0", skip_unboxed=True)
