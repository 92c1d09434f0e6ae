"""-m gpu: the opt-in f16 inference mode (`set_option("precision", 2)`: f16 operands, f32 accumulation, activations stored as
2 bytes; k_conv_mfma_f).

f16 rounding makes the result sensitive to the summation order (the CPU emulation, tests/f16_emulation.py, differs from ITSELF
by more than half of its error against the reference when run NCHW and channels_last), and the GPU kernel is a third order.  So
the GPU is judged against the REFERENCE (the repository's f32 oracle, first asserted to reproduce the fixtures' masks exactly)
with a margin derived from the emulation's own error E on the same frames: |gpu - ref| <= 2 E.  Why 2: the two CPU orders'
maxima differ by a few per cent from each other, the GPU's order is a third draw of the same error; a structural fault (a
dropped tap, chunk or channel half) shows as an error of the order of the activations, >= 50 x this bound.

Records printed by test_fixtures_* (not gates): flips per fixture, largest |reference logit| at a flip, largest relative area
error, per-frame Dice difference.
"""
import os

import numpy as np
import pytest

import f16_emulation as EMU
import head_cases as HC
import openglottal_amd as og
from openglottal_amd import synth
from oracle import layer_ref as R

pytestmark = pytest.mark.gpu


def make_model(sd, features, precision=2):
    m = og.UNet(1, 1, tuple(int(f) for f in features))
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    m.set_option("precision", precision)
    return m


def _unpack(bits, n):
    return np.unpackbits(bits, axis=1)[:, :65536].reshape(n, 256, 256)


_CACHE = {}


def fixture(golden_dir, name):
    """Frames, GT, weights, the f32 oracle's logits (asserted to give the fixture's masks exactly) and the emulation's E / D:
    CPU work, once per fixture and module."""
    if name in _CACHE:
        return _CACHE[name]
    clean, gt_c = synth.glottis_frames(4, 20, seed=99)
    if name == "unet_trained_small":
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        sd = {k[2:]: g[k] for k in g.files if k.startswith("W:")}
        frames, gt = clean, gt_c
    else:
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        g9 = np.load(os.path.join(golden_dir, "unet_trained_full.npz"))
        sd = {k[2:]: (g9[k].astype(np.float32) if g9[k].dtype == np.float16 else g9[k]) for k in g9.files if k.startswith("W:")}
        if name == "unet_trained_hard":
            sd = synth.detuned_weights(sd)
        hard, gt_h = synth.degraded_glottis_frames()
        frames, gt = np.concatenate([clean, hard]), np.concatenate([gt_c, gt_h])
    n = len(frames)
    assert n == len(g["areas"])
    ref = EMU.logits(sd, frames, half=False)
    ref_mask = EMU.masks_from_logits(ref)
    assert np.array_equal(ref_mask, _unpack(g["masks_packed"], n) > 0), (name, int((ref_mask != (_unpack(g["masks_packed"], n) > 0)).sum()))
    E, D, emu_a, emu_b = EMU.emulation_error(sd, frames, ref)
    emu_flips = int((EMU.masks_from_logits(emu_a) != ref_mask).sum())
    print(f"{name}: {n} frames, emulation E {E:.3g} (NCHW / channels_last), D {D:.3g}, max|logit| {np.abs(ref).max():.3g}, emulation flips {emu_flips}")
    fx = dict(name=name, feats=tuple(int(f) for f in g["features"]), sd=sd, frames=frames, gt=gt, ref=ref, ref_mask=ref_mask, E=E, D=D)
    _CACHE[name] = fx
    return fx


def judge(fx, mk, ar, lg, what, boxes=None):
    """The 2E rule on every pixel, mask == (prob_f32 > 0.5) -- the head's rule, tests/head_cases.py: decided on the rounded f32
    sigmoid, so a positive logit below 2^-25 is OFF, where `logits > 0` would say on --, area == popcount [in box],
    |area - ref area| <= flips, mean Dice."""
    ref, ref_mask, E, gt = fx["ref"][:len(lg)], fx["ref_mask"][:len(lg)], fx["E"], fx["gt"][:len(lg)]
    n = len(lg)
    err = float(np.abs(lg - ref).max())
    print(f"{fx['name']} {what}: max|gpu - ref| {err:.3g} = {err / E:.2f} E")
    assert err <= 2 * E, (what, err, E)
    on = mk > 0
    undecided = HC.check_mask_follows_the_rule(on, lg, what)           # off below 2^-25 (zero and negative included), on from 2^-21
    if undecided:
        print(f"{fx['name']} {what}: {undecided} logit(s) in [2^-25, 2^-21), where the last bits of expf decide")
    flips = on != ref_mask
    per = flips.reshape(n, -1).sum(1)
    if boxes is None:
        assert np.array_equal(ar.astype(np.int64), on.reshape(n, -1).sum(1)), what
        ref_area = ref_mask.reshape(n, -1).sum(1)
    else:
        want = [0 if b[0] < 0 else int(on[i][b[1]:b[3], b[0]:b[2]].sum()) for i, b in enumerate(boxes)]
        assert ar.tolist() == want, what
        ref_area = np.array([0 if b[0] < 0 else int(ref_mask[i][b[1]:b[3], b[0]:b[2]].sum()) for i, b in enumerate(boxes)])
    assert np.all(np.abs(ar.astype(np.int64) - ref_area) <= per), what
    at_flip = float(np.abs(ref[flips]).max()) if flips.any() else 0.0
    assert at_flip <= 2 * E, (what, at_flip)                      # (implied by the two assertions above; stated for the reader)
    if boxes is None:
        d_gpu = np.array([og.dice(mk[i], gt[i]) for i in range(n)])
        d_ref = np.array([og.dice(ref_mask[i].astype(np.uint8) * 255, gt[i]) for i in range(n)])
        assert abs(d_gpu.mean() - d_ref.mean()) <= 1e-3, (what, d_gpu.mean(), d_ref.mean())
        rel = float((np.abs(ar.astype(np.int64) - ref_area) / np.maximum(ref_area, 1)).max())
        print(f"{fx['name']} {what}: flips {int(per.sum())} of {n * 65536} (max {int(per.max())} per frame), largest |ref logit| at a flip {at_flip:.3g}, "
              f"largest relative area error {rel:.3g}, max per-frame |dDice vs GT| {float(np.abs(d_gpu - d_ref).max()):.3g}, "
              f"|d mean Dice| {abs(d_gpu.mean() - d_ref.mean()):.3g}")
    return err / E


def test_it_really_ran_the_f16_kernels(golden_dir):
    import torch

    fx = fixture(golden_dir, "unet_trained_small")
    m = make_model(fx["sd"], fx["feats"])
    m.set_chunk(64)
    fdev = torch.from_numpy(fx["frames"][:64]).cuda()
    k64 = [p["kernel"] for p in m.profile(fdev, 64, 256, 256, reps=1)]
    assert k64 and all(k.startswith(("k_conv_mfma_f", "k_sum_counts")) for k in k64), k64
    assert sum(k.startswith("k_conv_mfma_f") for k in k64) >= 21
    k1 = [p["kernel"] for p in m.profile(fdev, 1, 256, 256, reps=1)]
    assert all(k.startswith(("k_conv_mfma_f", "k_conv_first_f", "k_head_f", "k_sum_counts")) for k in k1), k1
    assert sum(k.startswith("k_conv_mfma_f") for k in k1) == 21, k1
    out = {}
    for prec in (2, 0, 1):
        m.set_option("precision", prec)
        _, _, out[prec] = m.segment(fx["frames"][:8], want_logits=True)
    assert not np.array_equal(out[2], out[0]) and not np.array_equal(out[2], out[1])      # no silent fall-back
    assert np.abs(out[2] - out[0]).max() <= 2 * fx["E"] + 1e-3
    with pytest.raises(og.OpenGlottalHipError):
        m.set_option("precision", 3)
    m.set_option("precision", 2)
    with pytest.raises(og.OpenGlottalHipError):      # the mode never splits K
        m.set_option("splitk", 1)


def test_every_layer_boundary_small_net_f16(golden_dir):
    g = np.load(os.path.join(golden_dir, "unet_small_layers.npz"))
    sd = synth.make_unet_state_dict(tuple(g["features"]), seed=int(g["seed"]), head_scale=float(g["head_scale"]), head_bias=float(g["head_bias"]))
    f = synth.random_gray_frames(1, 64, 64, seed=21)
    x = (f.astype("float32") / 255.0)[:, None]
    ta, tb = EMU.layer_taps(sd, x, True, False), EMU.layer_taps(sd, x, True, True)
    keys = [k[2:] for k in g.files if k.startswith("L:")]
    assert len(keys) == 27
    worst = 0.0
    for fuse in (0, 1):       # (the forward entry point keeps every tap: the fused head then stores the last activation too)
        m = make_model(sd, g["features"])
        m.set_option("fuse_head", fuse)
        logits = m(x)
        for k in keys:
            ref = g["L:" + k]
            got = logits if k == "head" else m.activation(k, 1)
            assert got.shape == ref.shape, (k, got.shape, ref.shape)
            El = max(float(np.abs(ta[k] - ref).max()), float(np.abs(tb[k] - ref).max()))
            err = float(np.abs(got - ref).max())
            print(f"layer {k:14s} fuse_head {fuse}: |gpu - ref| {err:.3g}  E_l {El:.3g}  ratio {err / El:.2f}")
            worst = max(worst, err / El)
            assert err <= 2 * El, (k, err, El)
            if k != "head":
                assert np.array_equal(got, got.astype(np.float16).astype(np.float32)), k      # stored values are f16 values
        # and each launch alone, from its own input tap, at half-ulp sharpness (oracle/layer_ref.py: check_f16)
        need = R.check_net(sd, f, lambda k: m.activation(k, 1), np.asarray(logits)[:, 0], R.kappa_of("f16"), form="f16")
        assert len(need) == 27
        layer = max(need, key=need.get)
        print(f"fuse_head {fuse}: smallest kappa each layer needs (of {R.KAPPA['f16']:g}): "
              + " ".join(f"{k}={v:.2f}" for k, v in need.items() if not k.startswith("pool")) + f"  (max {need[layer]:.2f} at {layer})")
    print(f"largest |gpu - ref| / E_l over the 27 tensors: {worst:.2f}")


@pytest.mark.parametrize("name", ["unet_trained_small", "unet_trained_full", "unet_trained_hard"])
def test_fixtures_in_bench_configuration_and_small_chunks(golden_dir, name):
    import torch

    fx = fixture(golden_dir, name)
    frames, n = fx["frames"], len(fx["frames"])
    m = make_model(fx["sd"], fx["feats"])
    m.set_chunk(64)
    m.set_graphs(True)
    m.set_option("dual", 1)
    dev = torch.device("cuda", 0)
    fdev = torch.from_numpy(frames).to(dev)
    area = torch.zeros(n, dtype=torch.int32, device=dev)
    mask = torch.zeros((n, 256, 256), dtype=torch.uint8, device=dev)
    logits = torch.zeros((n, 256, 256), dtype=torch.float32, device=dev)
    first = None
    for rep in range(2):          # graph capture, then replay
        m.segment_dev(fdev, n, 256, 256, area, mask_dev=mask, logits_dev=logits)
        m.sync()
        mk, ar, lg = mask.cpu().numpy(), area.cpu().numpy(), logits.cpu().numpy()
        judge(fx, mk, ar, lg, f"chunk 64, device pointers, pass {rep}")
        if first is None:
            first = lg.copy()
        assert np.array_equal(first, lg)
    for chunk in (1, 3):
        m.set_chunk(chunk)
        mk, ar, lg = m.segment(frames, want_logits=True)
        judge(fx, mk, ar, lg, f"chunk {chunk}, host")
        assert np.array_equal(lg, first), chunk
    m.set_chunk(64)
    boxes = np.array([og.utils.normalize_box((100, 80, 160, 200), 256, 256)] * 8, np.int32)
    boxes[5] = -1
    mk, ar, lg = m.segment(frames[:8], boxes=boxes, want_logits=True)
    judge(fx, mk, ar, lg, "boxes", boxes=boxes)


def test_logits_are_a_function_of_the_frame_only(golden_dir):
    import torch

    fx = fixture(golden_dir, "unet_trained_full")
    frames = fx["frames"][17:87]      # 70 frames: clean and degraded
    m = make_model(fx["sd"], fx["feats"])
    m.set_chunk(64)
    mk0, ar0, lg0 = m.segment(frames, want_logits=True)
    mk0b, ar0b, lg0b = m.segment(frames, want_logits=True)
    assert np.array_equal(lg0, lg0b) and np.array_equal(ar0, ar0b) and np.array_equal(mk0, mk0b)      # repeatable
    for chunk in (1, 3, 32, 64):
        for lanes in (1, 3):
            for graphs in (True, False):
                m.set_chunk(chunk); m.set_option("lanes", lanes); m.set_graphs(graphs)
                mk, ar, lg = m.segment(frames, want_logits=True)
                assert np.array_equal(lg, lg0) and np.array_equal(ar, ar0) and np.array_equal(mk, mk0), (chunk, lanes, graphs)
    m.set_option("lanes", 0); m.set_graphs(True)
    for chunk in (64, 3):
        for fh in (0, 1):
            for ff in (0, 1):
                m.set_chunk(chunk); m.set_option("fuse_head", fh); m.set_option("fuse_first", ff)
                mk, ar, lg = m.segment(frames, want_logits=True)
                assert np.array_equal(lg, lg0) and np.array_equal(ar, ar0) and np.array_equal(mk, mk0), (chunk, fh, ff)
    m.set_option("fuse_head", 1); m.set_option("fuse_first", 1)
    for chunk in (64, 3):
        m.set_chunk(chunk)
        for stream in (0, 1):
            m.set_option("stream", stream)
            mk, ar, lg = m.segment(frames, want_logits=True)
            assert np.array_equal(lg, lg0) and np.array_equal(ar, ar0), (chunk, stream)
        mks, ars = m.segment_stream(frames, want_mask=True)
        assert np.array_equal(mks, mk0) and np.array_equal(ars, ar0), chunk
        dev = torch.device("cuda", 0)
        d_f = torch.from_numpy(frames).to(dev)
        d_a = torch.zeros(70, dtype=torch.int32, device=dev)
        d_m = torch.zeros((70, 256, 256), dtype=torch.uint8, device=dev)
        d_l = torch.zeros((70, 256, 256), dtype=torch.float32, device=dev)
        for rep in range(2):
            m.segment_dev(d_f, 70, 256, 256, d_a, mask_dev=d_m, logits_dev=d_l)
            m.sync()
            assert np.array_equal(d_l.cpu().numpy(), lg0) and np.array_equal(d_a.cpu().numpy(), ar0) and np.array_equal(d_m.cpu().numpy(), mk0), (chunk, rep)
    # the f32 __call__ path (NCHW floats in) on the same frames: the same first-layer chain, the same bits
    assert np.array_equal(m((frames[:5].astype("float32") / 255.0)[:, None])[:, 0], lg0[:5])
    # and switching the precision back and forth on one handle re-plans the arena (2 / 4 bytes per channel)
    m.set_option("precision", 0)
    _, _, lg32 = m.segment(frames[:6], want_logits=True)
    m.set_option("precision", 2)
    _, _, lg16 = m.segment(frames[:6], want_logits=True)
    assert np.array_equal(lg16, lg0[:6]) and not np.array_equal(lg32, lg16)
    assert np.abs(lg32 - fx["ref"][17:23]).max() <= 1e-3


def test_odd_shapes_and_padded_channels_f16():
    from oracle import unet_oracle as O
    for feats, B, H, W, seed in [((32, 64, 128), 96, 80, 48, 321), ((33, 66), 128, 32, 64, 99), ((6, 12, 24), 2, 48, 32, 5)]:
        sd = synth.make_unet_state_dict(feats, seed=seed, head_scale=2.0, head_bias=-0.4)
        m = make_model(sd, feats)
        m.set_chunk(B)
        fr = synth.random_gray_frames(B, H, W, seed=17)
        masks, areas, logits = m.segment(fr, want_logits=True)
        masks2, areas2, logits2 = m.segment(fr, want_logits=True)
        assert np.array_equal(logits, logits2) and np.array_equal(areas, areas2)          # repeatable
        nref = min(B, 8)
        ref_mask, ref_logits = O.segment_frames(sd, fr[:nref], backend="torch")
        E, D, _, _ = EMU.emulation_error(sd, fr[:nref], ref_logits)
        err = float(np.abs(logits[:nref] - ref_logits).max())
        print(f"features {feats} {H}x{W}: |gpu - ref| {err:.3g}, E {E:.3g} (ratio {err / E:.2f}), D {D:.3g}, max|logit| {np.abs(ref_logits).max():.3g}")
        assert err <= 2 * E, (feats, err, E)
        assert np.all(np.abs(ref_logits[(masks[:nref] > 0) != (ref_mask > 0)]) <= 2 * E)
        assert np.array_equal(areas, (masks > 0).reshape(B, -1).sum(1))
        m.set_chunk(3)
        _, areas3, logits3 = m.segment(fr, want_logits=True)
        assert np.array_equal(logits3, logits) and np.array_equal(areas3, areas), feats


def test_resized_frames_device_and_host_compositions_agree_f16(golden_dir):
    from openglottal_amd.utils import unet_segment_frame, unet_segment_frame_host

    fx = fixture(golden_dir, "unet_trained_full")
    m = make_model(fx["sd"], fx["feats"])
    m.set_chunk(32)
    frames, _ = synth.glottis_frames(1, 3, h=480, w=640, seed=480 * 3 + 640)
    flips = 0
    for g in frames:
        dev = unet_segment_frame(g, m, None, 0.5)
        host = unet_segment_frame_host(g, m, None, 0.5)
        assert dev.shape == host.shape == (480, 640)
        diff = dev != host
        if diff.any():
            _, _, prob = m.segment_resized(g[None], threshold=0.5, want_prob=True)
            assert np.all(np.abs(prob[0][diff] - 0.5) <= 1e-6)
            flips += int(diff.sum())
        assert (dev > 0).any()
    print(f"f16 mode, 480x640: device vs host unet_segment_frame: {flips} flipped pixels")


def test_activation_beyond_the_f16_range_fails_loudly_in_f16_mode():
    """Finite, in-bounds data only: weights that push an activation beyond 60000 make the mode's result meaningless; that is an
    error (OG_ERANGE), never a silently saturated mask."""
    import torch

    feats = (32, 64)
    sd = synth.make_unet_state_dict(feats, seed=4, head_scale=2.0, head_bias=-0.3)
    big = dict(sd)
    big["downs.0.net.1.weight"] = (sd["downs.0.net.1.weight"] * np.float32(4e5)).astype(np.float32)   # first BN scale: activations ~1e5
    m = make_model(big, feats, precision=0)
    fr = synth.random_gray_frames(70, 32, 64, seed=3)
    m.set_chunk(64)
    _, _, logits = m.segment(fr, want_logits=True)          # exact f32: fine (finite logits)
    assert np.isfinite(logits).all()
    m.set_option("precision", 2)
    for chunk in (64, 2):                                   # fused first layer / separate first-layer kernel
        m.set_chunk(chunk)
        with pytest.raises(og.OpenGlottalHipError, match="f16 range"):
            m.segment(fr)
    with pytest.raises(og.OpenGlottalHipError, match="f16 range"):
        m((fr[:2].astype("float32") / 255.0)[:, None])
    d = torch.from_numpy(fr).cuda()
    a = torch.zeros(70, dtype=torch.int32, device="cuda")
    m.segment_dev(d, 70, 32, 64, a)                         # asynchronous entry point: reported by the sync
    with pytest.raises(og.OpenGlottalHipError, match="f16 range"):
        m.sync()
    m.sync()                                                # the flag is cleared by the report
    ok = make_model(sd, feats)                              # ordinary weights: no error
    ok.segment(fr)
    # the SAME handle works again once it is asked for something in range: exact f32 on the big weights
    m.set_option("precision", 0)
    _, _, again = m.segment(fr, want_logits=True)
    assert np.array_equal(again, logits)
