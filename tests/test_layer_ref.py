"""CPU: the per-layer float64 checker of oracle/layer_ref.py has power, and the GPU matrix covers what it claims.

* f32 arithmetic of every kernel form -- a torch-CPU f32 conv (the direct form), the numpy f32 Winograd emulation and the f16
  hi / lo emulation of split precision -- passes the check at its form's kappa, on the GPU matrix's nets scaled down;
* each mutant of a kernel's arithmetic, applied to ONE output element of an otherwise correct f32 result, is flagged;
* every case of tests/test_gpu_layer_parity.py runs the kernel families it is meant to exercise (og_unet_plan, no GPU needed).
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


# ───────────────────────────── coverage of the GPU matrix ─────────────────────────────


@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c["id"] for c in R.GPU_CASES])
def test_gpu_matrix_case_runs_the_kernels_it_claims(case):
    from test_launch_plan import check, plan

    recs, _ = plan(case["feats"], case["B"], case["H"], case["W"], 1, R.option_string(case["options"]))
    check(recs, case["id"])
    fams = R.plan_families(recs, case["B"])
    missing = set(case["families"]) - fams
    assert not missing, (case["id"], sorted(missing), sorted(fams))
    if case["fused_first"]:
        assert "first-fused" in fams and "k_conv_first" not in fams
    else:
        assert "first-fused" not in fams
    if case["fused_head"]:
        assert "k_head" not in fams and case["options"]["keep_taps"] == 0
