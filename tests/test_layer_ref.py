"""CPU: the per-layer float64 checker of oracle/layer_ref.py has power, and the GPU matrix covers what it claims.

* f32 arithmetic of every kernel form -- a torch-CPU f32 conv (the direct form), the numpy f32 Winograd emulation and the f16
  hi / lo emulation of split precision -- passes the check at its form's kappa, on the GPU matrix's nets scaled down;
* each mutant of a kernel's arithmetic, applied to ONE output element of an otherwise correct f32 result, is flagged;
* every case of tests/test_gpu_layer_parity.py runs the kernel families it is meant to exercise (og_unet_plan, no GPU needed);
* the f16 mode's form ("f16": an interval of f16 values per element, not a tolerance): its torch-CPU emulation passes at kappa 16,
  eleven mutants planted into one element each are flagged there, and the f16 rows of the matrix run, by instantiation, every
  kernel the mode can launch, with a half last chunk (ConvArgs::k_half) both alone and after full chunks;
* the f32 and split-precision chains likewise: layer_ref.F32_KERNELS lists every instantiation precision 0 and 1 can launch; an
  option sweep over og_unet_plan finds none outside it, every entry is reached, the non-f16 rows of the matrix run all of them, and
  whatever can run on a shape with edges is run on one.
"""
import numpy as np
import pytest

from oracle import layer_ref as R
from oracle import unet_oracle as O
from openglottal_amd import synth

FRAME_ORDER = ["mosaic", "random", "zeros", "full", "checker", "stripes"]

# the GPU matrix's nets, scaled down in frame size where float64 on the CPU is slow
EMU_NETS = [((32, 64), 32, 64), ((4, 8, 16, 32), 16, 16), ((3, 6, 12, 24, 48), 64, 96), ((33, 66), 32, 64), ((40, 80), 32, 32),
            ((32, 64, 128, 256), 32, 32)]


def frames_of(H, W, n=6, seed=1):
    sp = R.special_frames(H, W, seed=seed)
    return np.stack([sp[k] for k in FRAME_ORDER[:n]])


def emulate_chain(sd, gray, form):
    """f32 taps of the whole net with every 3x3 conv after the first layer in the emulated arithmetic of ``form``
    ("wino" | "split"); the first layer, the pools and the transposed convs in float64 rounded to f32 (hi / lo for split)."""
    L = O.n_levels(sd)
    q = (lambda v: R.join_hilo(*R.split_hilo(v))) if form == "split" else (lambda v: np.asarray(v, np.float32))
    taps = {}

    def conv(prefix, idx, x):
        s, sh, _ = R.fold_bn(sd, f"{prefix}.net.{idx + 1}")
        w = sd[f"{prefix}.net.{idx}.weight"]
        return R.wino_f32(x, w, s, sh) if form == "wino" else R.split_f32(x, w, s, sh)

    a = q(R.conv3_bn_relu(sd, "downs.0.net.0.weight", "downs.0.net.1", R.first_input(gray))[0])
    taps["downs.0.a"] = a
    for i in range(L):
        if i > 0:
            a = taps[f"downs.{i}.a"] = conv(f"downs.{i}", 0, taps[f"pool{i - 1}"])
        taps[f"downs.{i}.b"] = conv(f"downs.{i}", 3, a)
        taps[f"pool{i}"] = R.maxpool2(taps[f"downs.{i}.b"])
    taps["bottleneck.a"] = conv("bottleneck", 0, taps[f"pool{L - 1}"])
    x = taps["bottleneck.b"] = conv("bottleneck", 3, taps["bottleneck.a"])
    for j in range(L):
        i = L - 1 - j
        t = taps[f"ups.{2 * j}"] = q(R.convt(sd, f"ups.{2 * j}", x)[0])
        a = taps[f"ups.{2 * j + 1}.a"] = conv(f"ups.{2 * j + 1}", 0, np.concatenate([taps[f"downs.{i}.b"], t], 1))
        x = taps[f"ups.{2 * j + 1}.b"] = conv(f"ups.{2 * j + 1}", 3, a)
    logits = np.asarray(R.head(sd, x)[0][:, 0], np.float32)
    return taps, logits


def gpu_case_frames(H, W, n, seed=5):
    """The frames test_gpu_layer_parity.py reads back (its ``batch``): the special frames in ORDER, random seed 5."""
    sp = R.special_frames(H, W, seed=seed)
    return np.stack([sp[k] for k in FRAME_ORDER[:n]])


# plus the five-level net of the GPU matrix with that file's weights (seed 11) and frames: its downs.0.b is the hardest case
EMU_GPU_NETS = [((3, 6, 12, 24, 48), 64, 96, 4)]


def worst_of(form, kappa):
    out = {}
    nets = [(f, H, W, synth.make_unet_state_dict(f, seed=3), frames_of(H, W)) for f, H, W in EMU_NETS]
    nets += [(f, H, W, synth.make_unet_state_dict(f, seed=11, head_scale=3.0, head_bias=-0.5), gpu_case_frames(H, W, n))
             for f, H, W, n in EMU_GPU_NETS]
    for feats, H, W, sd, gray in nets:
        taps, logits = emulate_chain(sd, gray, form)
        w = R.check_net(sd, gray, taps.__getitem__, logits, kappa)
        conv_layers = {k: v for k, v in w.items() if k.endswith((".a", ".b")) and k != "downs.0.a"}   # the emulated 3x3 convs
        out[(feats, H, W)] = max(conv_layers.values()) * kappa["conv3"]     # as a multiple of 2^-24 M
    return out


def test_direct_f32_passes_at_its_kappa():
    """f32 arithmetic of every op through check_net at kappa_direct: the numpy f32 chain of unet_oracle.forward_numpy (it keeps
    every layer tap).  The torch-CPU f32 conv (oneDNN) is held to every form's kappa in test_mutant_is_flagged (its unmutated result)."""
    for feats, H, W in EMU_NETS:
        sd = synth.make_unet_state_dict(feats, seed=3)
        gray = frames_of(H, W)
        taps = {}
        logits = O.forward_numpy(sd, (gray.astype(np.float32) / 255.0)[:, None], taps)[:, 0]
        w = R.check_net(sd, gray, taps.__getitem__, logits, R.kappa_of("direct"))
        print(feats, H, W, "direct f32 worst |err|/bound %.3f" % max(w.values()))
        assert max(w.values()) <= 1.0


def test_winograd_emulation_passes_at_its_kappa():
    w = worst_of("wino", R.kappa_of("wino"))
    for k, v in w.items():
        print("winograd f32 emulation", k, "worst |err| / (2^-24 M) = %.2f" % v)
    worst = max(w.values())
    assert worst <= R.KAPPA["wino"]
    assert worst <= 2 * R.WINO_EMULATED_MAX, "the emulated figure the kappa was derived from has moved: re-derive kappa"


def test_split_precision_emulation_passes_at_its_kappa():
    w = worst_of("split", R.kappa_of("split"))
    for k, v in w.items():
        print("split-precision emulation", k, "worst |err| / (2^-24 M) = %.2f" % v)
    worst = max(w.values())
    assert worst <= R.KAPPA["split"]
    assert worst <= 2 * R.SPLIT_EMULATED_MAX, "the emulated figure the kappa was derived from has moved: re-derive kappa"


def f16_emulated_taps(sd, gray, channels_last):
    """The taps and logits of the f16 mode's torch-CPU emulation (tests/f16_emulation.py) under check_net's names."""
    import f16_emulation as EMU

    taps = EMU.layer_taps(sd, (gray.astype(np.float32) / 255.0)[:, None], True, channels_last)
    return taps, taps["head"][:, 0]


def test_f16_emulation_passes_at_its_kappa():
    """The f16 mode's emulation in both memory formats (two summation orders) through the interval check, on the matrix's nets
    scaled down, the five-level net of the GPU matrix with its own weights and frames, the six special frames; then the composed
    checks (no downs.0.a, no ups.N.b) on the same taps."""
    k = R.kappa_of("f16")
    nets = [(f, H, W, synth.make_unet_state_dict(f, seed=3), frames_of(H, W)) for f, H, W in EMU_NETS]
    nets += [(f, H, W, synth.make_unet_state_dict(f, seed=11, head_scale=3.0, head_bias=-0.5), gpu_case_frames(H, W, 6))
             for f, H, W, _ in EMU_GPU_NETS]
    stored, head, composed = 0.0, 0.0, 0.0
    for feats, H, W, sd, gray in nets:
        for cl in (False, True):
            taps, logits = f16_emulated_taps(sd, gray, cl)
            w = R.check_net(sd, gray, taps.__getitem__, logits, k, frames=FRAME_ORDER, form="f16")
            layer, worst = max(((n, v) for n, v in w.items() if n != "head"), key=lambda t: t[1])
            print(f"f16 emulation {feats} {H}x{W} channels_last={cl}: needs kappa {worst:.2f} ({layer}), head {w['head']:.2f}")
            stored, head = max(stored, worst), max(head, w["head"])
            hidden = {n: v for n, v in taps.items() if n not in ("downs.0.a", f"ups.{2 * len(feats) - 1}.b")}
            wc = R.check_net(sd, gray, hidden.__getitem__, logits, k, frames=FRAME_ORDER, form="f16", fused_first=True, fused_head=True)
            composed = max(composed, wc["downs.0.b (fused first)"], wc["head (fused)"])
    print(f"f16 emulation: stored tensors need kappa {stored:.2f}, the head {head:.2f}, the composed checks {composed:.2f}")
    assert stored <= R.KAPPA["f16"] and head <= R.KAPPA["f16"] and composed <= R.KAPPA["f16"]
    assert stored <= 2 * R.F16_EMULATED_MAX["stored"] and head <= 2 * R.F16_EMULATED_MAX["head"], \
        "the emulated figures the kappa was derived from have moved: re-derive kappa"


def test_composed_bounds_and_exact_checks_on_the_cpu_chain():
    """check_net's fused-first / fused-head compositions, the pool / mask / area exact checks, on a numpy f32 chain."""
    sd = synth.make_unet_state_dict((32, 64), seed=4, head_scale=3.0, head_bias=-0.5)
    gray = frames_of(32, 64)
    taps = {}
    logits = O.forward_numpy(sd, (gray.astype(np.float32) / 255.0)[:, None], taps)[:, 0]
    mask = ((O._sigmoid32(logits) > 0.5).astype(np.uint8) * 255)
    area = (mask > 0).reshape(len(mask), -1).sum(1)
    assert 0 < area.sum() < mask.size
    w = R.check_net(sd, gray, taps.__getitem__, logits, R.kappa_of("direct"), mask=mask, area=area, fused_first=True, fused_head=True)
    assert "downs.0.b (fused first)" in w and "head (fused)" in w and "downs.0.a" not in w
    bad = dict(taps)
    bad["pool1"] = taps["pool1"].copy()
    bad["pool1"][1, 3, 2, 2] = np.nextafter(bad["pool1"][1, 3, 2, 2], np.float32(np.inf))
    with pytest.raises(R.LayerMismatch, match=r"pool1: not bit-identical at frame 1 ch 3 \(y,x\)=\(2,2\)"):
        R.check_net(sd, gray, bad.__getitem__, logits, R.kappa_of("direct"))
    i, y, x = np.unravel_index(int(np.argmax(np.abs(logits) > 0.1)), logits.shape)
    m2 = mask.copy()
    m2[i, y, x] = 255 - m2[i, y, x]
    with pytest.raises(R.LayerMismatch, match="mask"):
        R.check_net(sd, gray, taps.__getitem__, logits, R.kappa_of("direct"), mask=m2)
    with pytest.raises(AssertionError, match="popcount"):
        R.check_net(sd, gray, taps.__getitem__, logits, R.kappa_of("direct"), mask=mask, area=area + 1)


# ───────────────────────────── mutants ─────────────────────────────


def _layer(feats=(33, 66), seed=6):
    """downs.1.net.0 of a (33, 66) net: 33 input channels (a padded 64-channel slot on the GPU), its input a ReLU'd f32 tensor."""
    sd = synth.make_unet_state_dict(feats, seed=seed)
    rs = np.random.RandomState(seed)
    x = np.maximum(rs.randn(1, feats[0], 16, 24), 0).astype(np.float32)
    return sd, x, "downs.1.net.0.weight", "downs.1.net.1"


def _plant(name, correct, mutated, ref, bound):
    """Put the mutant's value into ONE element of the correct result -- the element where the mutant is most visible -- and run
    the check; returns (ratio, element)."""
    r = np.abs(mutated.astype(np.float64) - ref) / bound
    idx = np.unravel_index(int(np.argmax(r)), r.shape)
    got = correct.copy()
    got[idx] = mutated[idx]
    with pytest.raises(R.LayerMismatch) as e:
        R.check(name, got, ref, bound)
    b, c, y, x = idx
    assert f"ch {c} (y,x)=({y},{x})" in str(e.value) and "1 element(s) over the bound" in str(e.value), str(e.value)
    return float(r[idx]), idx


def _correct_f32(sd, x, wk, bn):
    import torch
    import torch.nn.functional as F

    with torch.no_grad():
        y = F.conv2d(torch.from_numpy(x), torch.from_numpy(sd[wk]), None, 1, 1)
        p = bn
        y = F.batch_norm(y, torch.from_numpy(sd[p + ".running_mean"]), torch.from_numpy(sd[p + ".running_var"]),
                         torch.from_numpy(sd[p + ".weight"]), torch.from_numpy(sd[p + ".bias"]), False, 0.1, O.BN_EPS)
        return F.relu(y).numpy()


def _mutated(sd, x, wk, bn, delta_pre):
    s, shift, _ = R.fold_bn(sd, bn)
    pre = s[None, :, None, None] * R.conv3_raw(x, sd[wk]) + shift[None, :, None, None] + delta_pre
    return np.maximum(pre, 0).astype(np.float32)


MUTANTS = ["drop_input_channel", "padding_tap_from_neighbour", "padded_slot_last_channel", "split_a_lo_b_hi_dropped",
           "convt_dy_dx_swapped", "bn_eps_10x"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutant_is_flagged(mutant):
    sd, x, wk, bn = _layer()
    ref, _, M = R.conv3_bn_relu(sd, wk, bn, x)
    s, _, _ = R.fold_bn(sd, bn)
    sc = s[None, :, None, None]
    correct = _correct_f32(sd, x, wk, bn)
    forms = ["direct", "wino", "split"]
    if mutant in ("drop_input_channel", "padded_slot_last_channel"):
        c = 5 if mutant == "drop_input_channel" else x.shape[1] - 1        # 33 -> 32: the last real channel of the padded slot
        mutated = _mutated(sd, x, wk, bn, -sc * R.conv3_raw(x[:, c:c + 1], sd[wk][:, c:c + 1]))
    elif mutant == "padding_tap_from_neighbour":
        # at x = 0 the dx = 0 taps read the linear neighbour (the previous row's last pixel) instead of the zero padding
        H, W = x.shape[2:]
        xs = np.zeros_like(x, dtype=np.float64)
        xs[:, :, 1:, 0] = x[:, :, :-1, W - 1]
        d = np.zeros((1, sd[wk].shape[0], H, W))
        for dy in range(3):
            rows = np.arange(H) + dy - 1
            ok = (rows >= 0) & (rows < H)
            d[:, :, ok, 0] += np.einsum("oc,bch->boh", sd[wk][:, :, dy, 0].astype(np.float64), xs[:, :, rows[ok], 0])
        mutated = _mutated(sd, x, wk, bn, sc * d)
    elif mutant == "split_a_lo_b_hi_dropped":
        sh = R.fold_bn(sd, bn)[1]
        correct = R.split_f32(x, sd[wk], s, sh)
        mutated = R.split_f32(x, sd[wk], s, sh, drop="a_lo_b_hi")
        forms = ["split"]
    elif mutant == "convt_dy_dx_swapped":
        t = np.maximum(np.random.RandomState(2).randn(1, sd["ups.0.weight"].shape[0], 6, 8), 0).astype(np.float32)
        ref, M = R.convt(sd, "ups.0", t)
        w = sd["ups.0.weight"]
        import torch
        import torch.nn.functional as F

        correct = F.conv_transpose2d(torch.from_numpy(t), torch.from_numpy(w), torch.from_numpy(sd["ups.0.bias"]), 2).numpy()
        ws = np.ascontiguousarray(w.transpose(0, 1, 3, 2))
        mutated = (R.convt_raw(t, ws) + sd["ups.0.bias"].astype(np.float64)[None, :, None, None]).astype(np.float32)
        forms = ["direct", "split"]
    elif mutant == "bn_eps_10x":
        mutated = R.conv3_bn_relu(sd, wk, bn, x, eps=10 * O.BN_EPS)[0].astype(np.float32)
    ratios = {}
    for f in forms:
        bound = R.bound_of(M, R.KAPPA[f])
        assert R.check(mutant + " (correct)", correct, ref, bound) <= 1.0       # the unmutated result passes
        ratios[f], idx = _plant(mutant, correct, mutated, ref, bound)
    print(mutant, "flagged at element", idx, "|err|/bound:", {f: round(v, 2) for f, v in ratios.items()})


# ───────────────────────────── mutants of the f16 mode ─────────────────────────────


def _q16(v):
    return np.asarray(v, np.float32).astype(np.float16).astype(np.float32)


def _toward_zero16(v):
    """f32 -> f16 by truncation (round toward zero), as f32."""
    v = np.asarray(v, np.float32)
    r = v.astype(np.float16)
    over = np.abs(r.astype(np.float32)) > np.abs(v)
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float32)


def _f16_layer(feats=(33, 66), seed=6):
    """As ``_layer``, with the input an f16 tensor (what an f16-mode layer reads)."""
    sd, x, wk, bn = _layer(feats, seed)
    return sd, _q16(x), wk, bn


def _f16_conv(sd, x, wk, bn, w=None, eps=O.BN_EPS, store=_q16):
    """The f16 mode's conv3 + BN + ReLU on the CPU: torch f32 accumulation of exact products, one rounding at the store."""
    sdm = dict(sd)
    sdm[wk] = _q16(sd[wk]) if w is None else np.asarray(w, np.float32)
    import torch
    import torch.nn.functional as F

    with torch.no_grad():
        y = F.conv2d(torch.from_numpy(x), torch.from_numpy(sdm[wk]), None, 1, 1)
        y = F.batch_norm(y, torch.from_numpy(sd[bn + ".running_mean"]), torch.from_numpy(sd[bn + ".running_var"]),
                         torch.from_numpy(sd[bn + ".weight"]), torch.from_numpy(sd[bn + ".bias"]), False, 0.1, eps)
        return store(F.relu(y).numpy())


def _plant_f16(name, correct, mutated, ref, e, idx=None):
    """One element of the correct f16 result replaced by the mutant's -- the element where it shows most -- must be flagged there."""
    need = R.f16_needed(mutated, ref) / e
    if idx is None:
        idx = tuple(int(v) for v in np.unravel_index(int(np.argmax(need)), need.shape))
    got = correct.copy()
    got[idx] = mutated[idx]
    with pytest.raises(R.LayerMismatch) as err:
        R.check_f16(name, got, ref, e)
    b, c, y, x = idx
    assert f"ch {c} (y,x)=({y},{x})" in str(err.value) and "1 element(s) outside the interval" in str(err.value), str(err.value)
    outside = (mutated < R.rne16(ref - e)) | (mutated > R.rne16(ref + e))
    return float(need[idx]) * R.KAPPA["f16"], idx, float(outside.mean())


F16_MUTANTS = ["store_toward_zero", "one_ulp_high", "weights_left_f32", "weights_truncated", "k_half_chunk_dropped",
               "padded_slot_last_channel", "padding_tap_from_neighbour", "convt_dy_dx_swapped", "bn_eps_10x", "head_from_unrounded",
               "pool_one_ulp_off"]


@pytest.mark.parametrize("mutant", F16_MUTANTS)
def test_f16_mutant_is_flagged(mutant):
    kap = R.KAPPA["f16"]
    sd, x, wk, bn = _f16_layer((96, 192), 8) if mutant == "k_half_chunk_dropped" else _f16_layer()
    sd16 = R.f16_weights(sd)
    assert np.array_equal(sd16[wk], _q16(sd[wk])) and not np.array_equal(sd16[wk], sd[wk])
    assert all(np.array_equal(sd16[k], sd[k]) for k in sd if k.startswith("head.") or ".net." in k and not k.endswith(("0.weight", "3.weight")))
    assert np.array_equal(sd16["downs.0.net.0.weight"], sd["downs.0.net.0.weight"])
    ref, _, M = R.conv3_bn_relu(sd16, wk, bn, x)
    e = R.bound_of(M, kap)
    correct = _f16_conv(sd, x, wk, bn)
    s, _, _ = R.fold_bn(sd, bn)
    sc = s[None, :, None, None]
    idx = None

    def pre_shifted(delta):   # the float64 result with ``delta`` added before the ReLU, rounded once
        pre = sc * R.conv3_raw(x, sd16[wk]) + R.fold_bn(sd, bn)[1][None, :, None, None] + delta
        return _q16(np.maximum(pre, 0))

    if mutant == "store_toward_zero":
        mutated = _f16_conv(sd, x, wk, bn, store=_toward_zero16)
    elif mutant == "one_ulp_high":
        single = (R.rne16(ref - e) == R.rne16(ref + e)) & (ref > 0)
        print("positive outputs whose interval holds exactly one f16 value: %.1f %%" % (100.0 * single.sum() / (ref > 0).sum()))
        assert single.sum() > 0.8 * (ref > 0).sum()
        idx = tuple(int(v) for v in np.argwhere(single)[len(np.argwhere(single)) // 2])
        mutated = np.nextafter(correct.astype(np.float16), np.float16(np.inf)).astype(np.float32)
    elif mutant == "weights_left_f32":
        mutated = _f16_conv(sd, x, wk, bn, w=sd[wk])
    elif mutant == "weights_truncated":
        mutated = _f16_conv(sd, x, wk, bn, w=_toward_zero16(sd[wk]))
    elif mutant == "k_half_chunk_dropped":
        assert x.shape[1] == 96          # one full 64-channel chunk and a half one: channels 64..95 never accumulated
        mutated = pre_shifted(-sc * R.conv3_raw(x[:, 64:], sd16[wk][:, 64:]))
    elif mutant == "padded_slot_last_channel":
        c = x.shape[1] - 1               # 33 channels: index 32, the only real channel of the half chunk
        mutated = pre_shifted(-sc * R.conv3_raw(x[:, c:c + 1], sd16[wk][:, c:c + 1]))
    elif mutant == "padding_tap_from_neighbour":
        H, W = x.shape[2:]
        xs = np.zeros_like(x, dtype=np.float64)
        xs[:, :, 1:, 0] = x[:, :, :-1, W - 1]
        d = np.zeros((1, sd[wk].shape[0], H, W))
        for dy in range(3):
            rows = np.arange(H) + dy - 1
            ok = (rows >= 0) & (rows < H)
            d[:, :, ok, 0] += np.einsum("oc,bch->boh", sd16[wk][:, :, dy, 0].astype(np.float64), xs[:, :, rows[ok], 0])
        mutated = pre_shifted(sc * d)
    elif mutant == "convt_dy_dx_swapped":
        t = _q16(np.maximum(np.random.RandomState(2).randn(1, sd["ups.0.weight"].shape[0], 6, 8), 0))
        ref, M = R.convt(sd16, "ups.0", t)
        e = R.bound_of(M, kap)
        import torch
        import torch.nn.functional as F

        correct = _q16(F.conv_transpose2d(torch.from_numpy(t), torch.from_numpy(sd16["ups.0.weight"]), torch.from_numpy(sd["ups.0.bias"]), 2).numpy())
        ws = np.ascontiguousarray(sd16["ups.0.weight"].transpose(0, 1, 3, 2))
        mutated = _q16(R.convt_raw(t, ws) + sd["ups.0.bias"].astype(np.float64)[None, :, None, None])
    elif mutant == "bn_eps_10x":
        mutated = _f16_conv(sd, x, wk, bn, eps=10 * O.BN_EPS)
    elif mutant == "head_from_unrounded":
        # the f32 logits are held to the magnitude check from the STORED (rounded) last activation
        sdh = synth.make_unet_state_dict((33, 66), seed=6, head_scale=3.0, head_bias=-0.5)
        act32 = np.maximum(np.random.RandomState(3).randn(1, 33, 16, 24), 0).astype(np.float32)    # the f32 value before its rounding
        stored = _q16(act32)
        ref_h, M_h = R.head(sdh, stored)
        bound = R.bound_of(M_h, kap)
        good = ref_h.astype(np.float32)
        assert R.check("head (correct)", good, ref_h, bound) <= 1.0
        ratio, idx = _plant(mutant, good, R.head(sdh, act32)[0].astype(np.float32), ref_h, bound)
        print(mutant, "flagged at element", idx, "|err|/bound: %.1f" % ratio)
        return
    elif mutant == "pool_one_ulp_off":
        # pool of a tensor one f16 ulp off in one element (the maximum of its window): bit-exact check against maxpool2 of the stored tensor
        pooled = R.maxpool2(correct)
        y, xx = 4, 6
        win = correct[0, 2, 2 * y:2 * y + 2, 2 * xx:2 * xx + 2]
        off = correct.copy()
        iy, ix = np.unravel_index(int(np.argmax(win)), win.shape)
        off[0, 2, 2 * y + iy, 2 * xx + ix] = np.nextafter(np.float16(win.max()), np.float16(np.inf))
        R.check_exact("pool1", pooled, R.maxpool2(correct))
        with pytest.raises(R.LayerMismatch, match=rf"pool1: not bit-identical at frame 0 ch 2 \(y,x\)=\({y},{xx}\)"):
            R.check_exact("pool1", R.maxpool2(off), R.maxpool2(correct))
        return
    assert R.check_f16(mutant + " (correct)", correct, ref, e) <= kap      # the unmutated result passes
    need, idx, frac = _plant_f16(mutant, correct, mutated, ref, e, idx)
    print(mutant, "flagged at element", idx, "needs kappa %.3g; all elements outside if applied everywhere: %.1f %%" % (need, 100 * frac))


def test_check_f16_refuses_values_that_are_not_f16_and_non_finite_ones():
    sd, x, wk, bn = _f16_layer()
    ref, _, M = R.conv3_bn_relu(R.f16_weights(sd), wk, bn, x)
    e = R.bound_of(M, R.KAPPA["f16"])
    good = _f16_conv(sd, x, wk, bn)
    idx = np.unravel_index(int(np.argmax(ref)), ref.shape)
    bad = good.copy()
    bad[idx] = np.float32(ref[idx])                     # the better value, but not one the f16 store can hold
    assert bad[idx] != good[idx]
    with pytest.raises(R.LayerMismatch, match="is not an f16 value"):
        R.check_f16("layer", bad, ref, e)
    bad[idx] = np.inf
    with pytest.raises(R.LayerMismatch, match="non-finite"):
        R.check_f16("layer", bad, ref, e)
    # subnormal f16 references are ordinary values: a flushed one is flagged, the kept one passes
    tiny = np.full((1, 1, 1, 2), 3 * 2.0 ** -24)
    et = R.bound_of(tiny, R.KAPPA["f16"])
    assert R.check_f16("subnormal", tiny.astype(np.float32), tiny, et) == 0.0
    with pytest.raises(R.LayerMismatch, match="outside its f16 interval"):
        R.check_f16("subnormal", np.zeros((1, 1, 1, 2), np.float32), tiny, et)


# ───────────────────────────── coverage of the GPU matrix ─────────────────────────────


_MATRIX = R.GPU_CASES + R.F32_ENTRY_CASES


@pytest.mark.parametrize("case", _MATRIX, ids=[c["id"] for c in _MATRIX])
def test_gpu_matrix_case_runs_the_kernels_it_claims(case):
    from test_launch_plan import check, plan

    recs, _ = plan(case["feats"], case["B"], case["H"], case["W"], 1, R.option_string(case["options"]))
    check(recs, case["id"])
    if case["form"] == "f16":      # by instantiation: the text og_unet_plan records for each f16 launch
        assert case["options"]["precision"] == 2
        insts = R.plan_instantiations(recs)
        missing = set(case["families"]) - insts
        assert not missing, (case["id"], sorted(missing), sorted(insts))
        first, first_fused, head = (R.F16_KERNELS[k][0] for k in ("k_conv_first_f", "<1,0,8,3,FIRST>", "k_head_f"))
        assert (first_fused in insts) == case["fused_first"] and (first in insts) != case["fused_first"], (case["id"], sorted(insts))
        if case["fused_head"]:
            assert head not in insts and case["options"]["keep_taps"] == 0
        assert all("k_conv_mfma_f<" in r["kernel"] for r in recs if "k_conv" in r["kernel"] and "k_conv_first" not in r["kernel"])
        assert set(case["prof"]) <= {v[1] for v in R.F16_KERNELS.values()}
        return
    fams = R.plan_families(recs, case["B"])
    missing = set(case["families"]) - fams
    assert not missing, (case["id"], sorted(missing), sorted(fams))
    if case["fused_first"]:
        assert "first-fused" in fams and "k_conv_first" not in fams
    else:
        assert "first-fused" not in fams
    if case["fused_head"]:
        assert "k_head" not in fams and case["options"]["keep_taps"] == 0
    # by instantiation, exactly: the row claims every kernel its plan shows and no other
    assert case["kernels"], case["id"]
    claimed = {R.F32_KERNELS[k][0] for k in case["kernels"]}
    insts = R.plan_instantiations(recs)
    assert claimed == insts, (case["id"], "claimed, not planned:", sorted(claimed - insts), "planned, not claimed:", sorted(insts - claimed))
    assert set(case["prof_inst"]) == {R.F32_KERNELS[k][1] for k in case["kernels"]} - {None}
    assert (case["form"] == "split") == (case["options"].get("precision", 0) == 1)


# ───────────────────────────── the f32 and split-precision instantiations: a closed list ─────────────────────────────

SWEEP_BATCHES = (1, 2, 3, 8, 64)
# test_launch_plan.py's shapes (the full-width net at 256 x 256 first), then the other edge shapes of the GPU matrix
SWEEP_SHAPES = [(R.FULL, (256, 256)), ((32, 64), (128, 256)), ((32, 64), (96, 160)), ((64, 128), (48, 64)), ((40, 80), (64, 64)),
                ((32, 64, 128), (64, 32)), ((4, 8, 16, 32), (256, 256)), ((32, 64, 128, 256), (512, 512)),
                ((16, 32, 64, 128, 256), (256, 256)), ((96, 192), (64, 128)),
                ((33, 66), (32, 64)), ((4, 8, 16, 32), (16, 16)), ((4, 8, 16, 32), (16, 256)), ((3, 6, 12, 24, 48), (64, 96)),
                ((32, 64), (64, 64)), ((32, 64), (512, 512)), ((33, 66), (64, 64)), (R.FULL, (64, 64))]
SWEEP_SINGLE = ([f"conv_impl={v}" for v in (0, 1, 2, 3)] + [f"tps_nt1={v}" for v in (1, 3, 9)] + [f"tps_nt2={v}" for v in (1, 3)]
                + [f"tile_h={v}" for v in (0, 8, 16)] + [f"{n}={v}" for n in ("h_square", "convt_occ", "convt_w", "splitk_occ", "fuse_head",
                                                                              "fuse_first", "wino_first") for v in (0, 1)]
                + [f"occ_min_pct={v}" for v in (0, 400)] + [f"wg_per_cu={v}" for v in (1, 2)])
# each single value alone (the default Winograd chain) and on top of the other three chains
SWEEP_BASES = ["", "wino=0", "wino=0,conv_impl=1", "precision=1"]
_sweep_cache = {}


def sweep_option_sets():
    from test_launch_plan import OPTION_SETS

    out = list(OPTION_SETS)
    for base in SWEEP_BASES:
        out += [(base + "," if base else "") + s for s in SWEEP_SINGLE if s.split("=")[0] + "=" not in base]
    # split K on the persistent kernel: conv_impl 1, or the occupancy kernel's K parts switched off, and the tap groups under it
    out += ["conv_impl=1,splitk=1", "wino=0,conv_impl=1,splitk=1", "splitk=1,splitk_occ=0", "wino=0,splitk=1,splitk_occ=0",
            "wino=0,conv_impl=1,splitk=1,tps_nt1=1", "wino=0,conv_impl=1,splitk=1,tps_nt1=9,tps_nt2=3", "wino=0,conv_impl=1,splitk=1,tile_h=16",
            "precision=1,conv_impl=1,splitk=1", "wino=0,conv_impl=0,splitk=1", "wino=0,conv_impl=3,splitk=1"]
    out += ["entry_f32=1", "precision=1,entry_f32=1"]
    return list(dict.fromkeys(out))


def sweep():
    """{instantiation: [(is_edge, feats, H, W, B, options), ...]} over SWEEP_SHAPES x sweep_option_sets() x SWEEP_BATCHES (computed once)."""
    from test_launch_plan import plan

    if not _sweep_cache:
        for feats, (H, W) in SWEEP_SHAPES:
            edge = R.is_edge_case(dict(feats=feats, H=H, W=W))
            for options in sweep_option_sets():
                for B in SWEEP_BATCHES:
                    recs, _ = plan(feats, B, H, W, 1, options)
                    for inst in R.plan_instantiations(recs):
                        _sweep_cache.setdefault(inst, []).append((edge, feats, H, W, B, options))
    return _sweep_cache


def matrix_cover():
    """({instantiation: [row ids]}, the same over the edge rows only) from the PLANS of the non-f16 rows and the float entry cases."""
    from test_launch_plan import plan

    every, edges = {}, {}
    for c in _MATRIX:
        if c["form"] == "f16":
            continue
        recs, _ = plan(c["feats"], c["B"], c["H"], c["W"], 1, R.option_string(c["options"]))
        for inst in R.plan_instantiations(recs):
            every.setdefault(inst, []).append(c["id"])
            if R.is_edge_case(c):
                edges.setdefault(inst, []).append(c["id"])
    return every, edges


def test_f32_registry_is_closed_under_the_option_sweep():
    """No plan of the sweep shows an f32 or split-precision instantiation F32_KERNELS does not know, and no entry is dead: each is
    reached by the net, shape, micro-batch and option set it names."""
    from test_launch_plan import plan

    texts = {v[0] for v in R.F32_KERNELS.values()}
    assert len(texts) == len(R.F32_KERNELS) == 67
    assert not any(t.startswith(("k_conv_mfma_f<", "k_conv_first_f", "k_head_f")) for t in texts)
    seen = sweep()
    unknown = {i: w[0][1:] for i, w in seen.items() if i not in texts}
    assert not unknown, ("instantiations the registry does not know, and a plan that shows each", unknown)
    for short, (text, label, (feats, H, W, B, options)) in R.F32_KERNELS.items():
        assert "precision=2" not in options
        recs, _ = plan(feats, B, H, W, 1, options)
        assert text in R.plan_instantiations(recs), (short, text, "is not reached by", (feats, H, W, B, options))
        assert (label is None) == text.startswith("k_splitk_epilogue"), short
    # the sweep alone reaches all but the two that need three options at once (16-row persistent tiles with other tap groups)
    # -- those are reached by their own entries above
    assert texts - set(seen) <= {R.F32_KERNELS[k][0] for k in ("p<1,0,16,9>", "p<2,0,16,3>")}, sorted(texts - set(seen))


def test_f32_matrix_runs_every_registered_instantiation():
    """The union of instantiations over the plans of the non-f16 rows (and the float entry cases) IS the registry: dropping a row
    that is the only cover of an instantiation fails here and names it."""
    every, _ = matrix_cover()
    texts = {v[0] for v in R.F32_KERNELS.values()}
    assert set(every) == texts, ("never compared with float64:", sorted(texts - set(every)), "unregistered:", sorted(set(every) - texts))
    # and each is claimed, so that the GPU test asserts its UNet.profile label
    claimed = {k for c in _MATRIX for k in c["kernels"]}
    assert claimed == set(R.F32_KERNELS), sorted(set(R.F32_KERNELS) ^ claimed)
    for k in ("h<1,0,8,3,FIRST>", "h<1,0,8,3>", "o<1,0,16,2>", "p<1,0,16,3>", "p<2,0,16,1>", "p<1,0,16,9>", "p<2,0,16,3>", "p<1,0,8,9>",
              "p<2,0,8,3>", "p<1,0,8,1>", "ps<1,1>", "ps<1,2>", "ps<1,4>", "o<1,0,8,4>", "o<2,0,8,4>", "h<2,0,16,2>", "first<f32>",
              "first<f32,split>"):
        assert any(R.F32_KERNELS[k][1] in c["prof_inst"] for c in _MATRIX if k in c["kernels"]), k


def test_rows_redundant_for_coverage_are_exactly_the_listed_ones():
    """Every row added with the registry is the only cover of some instantiation -- overall or among the edge rows -- so that dropping
    it fails one of the two tests around this one by name; the exceptions are listed, with what each adds, in REDUNDANT_FOR_COVERAGE."""
    every, edges = matrix_cover()
    ids = [c["id"] for c in R.GPU_CASES if c["form"] != "f16"]
    new_rows = ids[ids.index("persistent-tps9-33x66"):]
    sole = {rows[0] for rows in list(every.values()) + list(edges.values()) if len(rows) == 1}
    redundant = {r for r in new_rows if r not in sole}
    assert redundant == set(R.REDUNDANT_FOR_COVERAGE), (sorted(redundant - set(R.REDUNDANT_FOR_COVERAGE)), sorted(set(R.REDUNDANT_FOR_COVERAGE) - redundant))
    assert all(R.REDUNDANT_FOR_COVERAGE.values())


def test_f32_matrix_covers_every_instantiation_on_an_edge_shape():
    """Whatever the planner can choose on a shape with edges (anything but the full-width net at 256 x 256: tiles with borders,
    padded channels, small maps) is judged on one: every instantiation the sweep -- or a registry entry's own option set -- reaches
    on an edge shape is run by at least one edge row.  EDGE_EXEMPT may list what the planner picks at 256 x 256 full width only."""
    _, edges = matrix_cover()
    on_edges = {i: next(w[1:] for w in where if w[0]) for i, where in sweep().items() if any(w[0] for w in where)}
    for text, _, (feats, H, W, B, options) in R.F32_KERNELS.values():
        if R.is_edge_case(dict(feats=feats, H=H, W=W)):
            on_edges.setdefault(text, (feats, H, W, B, options))
    for text, rule in R.EDGE_EXEMPT.items():
        assert text not in on_edges, (text, "is exempt but reachable on an edge shape:", on_edges[text])
        assert rule
    lost = {i: w for i, w in on_edges.items() if i not in edges}
    assert not lost, ("reachable on an edge shape but judged by no edge row (instantiation: a plan that reaches it)", lost)
    # every split-precision kernel is among them: partial tiles, padded channels and the 1 x 1 bottleneck at kappa * 2^-24 * M
    assert all(t in edges for t in (v[0] for v in R.F32_KERNELS.values()) if "k_conv_mfma_h" in t)
    split_edge = [c for c in R.GPU_CASES if c["form"] == "split" and R.is_edge_case(c)]
    assert {(c["feats"], c["H"], c["W"]) for c in split_edge} >= {((32, 64), 96, 160), ((33, 66), 32, 64), ((4, 8, 16, 32), 16, 16),
                                                                 ((3, 6, 12, 24, 48), 64, 96)}


def test_f16_matrix_covers_every_instantiation_and_both_half_chunks():
    """Over the f16 rows: every kernel instantiation the library can launch in the f16 mode (the list of its launch sites:
    launch_conv_f's six, the fused first layer, the first-layer and head kernels), and a half last chunk (ConvArgs::k_half) both
    as the only chunk of a layer and after full 64-channel chunks."""
    from test_launch_plan import plan

    cases = [c for c in R.GPU_CASES if c["form"] == "f16"]
    assert len(cases) == 15 and all(c["options"]["precision"] == 2 for c in cases)
    claimed, seen, halves = set(), set(), {}
    for c in cases:
        recs, _ = plan(c["feats"], c["B"], c["H"], c["W"], 1, R.option_string(c["options"]))
        claimed |= set(c["families"])
        seen |= R.plan_instantiations(recs)
        for kind in R.plan_half_chunks(recs):
            halves.setdefault(kind, []).append(c["id"])
    every = {v[0] for v in R.F16_KERNELS.values()}
    assert len(every) == 9
    assert claimed == every, sorted(every - claimed)
    assert seen == every, sorted(seen ^ every)          # and the plans show no f16 kernel the list does not know
    assert set(halves) == {"only", "after-full"}, halves
    assert "f16-padded-33x66-32x64" in halves["after-full"]     # the 96- and 160-channel layers
    # the existing helper is untouched by the f16 labels: it still reports families, not instantiations
    recs, _ = plan(R.FULL, 2, 256, 256, 1, "precision=2")
    assert "k_conv_mfma_f" in R.plan_families(recs, 2) and "first-fused" not in R.plan_families(recs, 2)

