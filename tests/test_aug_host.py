"""The host twin of the device augmentation (og_aug_stage_host, og_aug_apply_host, og_aug_noise_host), stage by stage against torch on
the CPU, each stage fed the twin's own previous output; `augment.draw` against a plain restatement of the reference's order.  No GPU."""
import math
import random

import numpy as np
import pytest
import torch

import aug_cases as AC
from openglottal_amd import augment as A

U = 2.0 ** -24                                                                # half an ulp of a value in [1, 2): one f32 rounding of a value <= 1


def planes(S, n=0):
    """a sample as the stages see it: I = u8 / 255 in f32, M = (u8 > 0)"""
    im, mk = AC.tiles(S)
    return im[n].astype(np.float32) / np.float32(255.0), (mk[n] > 0).astype(np.uint8)


@pytest.mark.parametrize("S", AC.SIZES)
def test_flips_are_exact(S):
    I, M = planes(S, 1)
    for h in (False, True):
        for v in (False, True):
            oi, om = A.stage_host("flip", I, M, A.record(hflip=h, vflip=v))
            dims = [d for d, on in ((1, h), (0, v)) if on]
            assert np.array_equal(oi, np.flip(I, dims) if dims else I) and np.array_equal(om, np.flip(M, dims) if dims else M), (h, v)


@pytest.mark.parametrize("S,angle", [(S, a) for S in AC.SIZES for a in AC.angles(S)])
def test_rotate_against_grid_sample(S, angle):
    I, M = planes(S, 3)
    oi, om = A.stage_host("rotate", I, M, A.record(angle=angle))
    ref = AC.torch_rotate(I, angle, "bilinear")
    err = float(np.abs(oi - ref).max())
    # a source coordinate is an f32 of magnitude < S computed in a handful of operations: a few ulp(S) = S 2^-23 each, in the twin and
    # in torch; the bilinear surface has a gradient of at most 1 per pixel and axis for taps in [0, 1]: 8 S 2^-23
    bound = 8 * S * 2.0 ** -23
    print(f"rotate S={S} angle={angle}: max |twin - grid_sample| = {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    sx, sy = AC.source_coordinates(S, angle)
    clear = (np.abs(sx - np.floor(sx) - 0.5) > 1e-3) & (np.abs(sy - np.floor(sy) - 0.5) > 1e-3)   # away from a tie of the rounding
    assert clear.mean() >= 0.99, clear.mean()
    refm = AC.torch_rotate(M.astype(np.float32), angle, "nearest")
    assert np.array_equal(om[clear].astype(np.float32), refm[clear])
    if angle == 0:                                                            # the identity, through the rule: exact
        assert np.array_equal(oi, I) and np.array_equal(om, M)


def test_nearest_ties_go_to_the_even_index():
    """No rotation puts a whole row on ties, but the record cos_t = sin_t = 1 does: in row S / 2 (Y = 0.5) the source index of column j
    is (j - 0.5, j + 0.5) exactly.  Source x = 0.5, 1.5, 2.5, 3.5 must read columns 0, 2, 2, 4."""
    S = 32
    M = np.zeros((S, S), np.uint8)
    rec = A.record()
    rec["cos_t"] = rec["sin_t"] = 1.0
    i = S // 2
    for col in range(6):
        M[:] = 0
        M[:, col] = 1                                                         # which outputs of row i read column `col`?
        om = A.stage_host("rotate", np.zeros((S, S), np.float32), M, rec)[1]
        got = [j for j in range(1, 5) if om[i, j]]
        assert got == [j for j, src in zip(range(1, 5), (0, 2, 2, 4)) if src == col], (col, got)


@pytest.mark.parametrize("S", AC.SIZES)
def test_rescale_against_interpolate(S):
    I, M = planes(S, 3)
    for new_size in (int(0.85 * S), S - 1, S, S + 1, int(1.15 * S)):
        oi, om = A.stage_host("rescale", I, M, A.record(new_size=new_size))
        assert np.array_equal(om.astype(np.float32), AC.torch_rescale(M.astype(np.float32), new_size, "nearest")), new_size   # bit for bit
        ref = AC.torch_rescale(I, new_size, "bilinear")
        err = float(np.abs(oi - ref).max())
        # per pass sum(w_k v_k), n taps, v in [0, 1], sum(w) = 1: a weight takes 4 roundings and the n of its divisor's sum,
        # (n + 4) U relative; the products and adds n U more: (2 n + 4) U per pass and side, two passes, two sides.  n <= 4 at these scales
        # (support max(in/out, 1) <= 1.18: int(c + 1.68) - int(c - 0.68) <= 4).
        bound = 4 * (2 * 4 + 4) * U
        print(f"rescale S={S} -> {new_size}: max |twin - interpolate| = {err:.3g} (bound {bound:.3g})")
        assert err <= bound
        pad = S - new_size
        if pad > 0:                                                           # the zero border: pl left and top, pad - pl right and bottom
            pl = pad // 2
            inner = np.zeros((S, S), bool)
            inner[pl:pl + new_size, pl:pl + new_size] = True
            assert not oi[~inner].any() and not om[~inner].any()
        if new_size == S:                                                     # the identity, through the bilinear rule: exact
            assert np.array_equal(oi, I) and np.array_equal(om, M)


@pytest.mark.parametrize("S", AC.SIZES)
@pytest.mark.parametrize("ks,sigma", [(3, 0.5), (3, 1.5), (5, 0.5), (5, 1.5)])
def test_blur_against_conv2d(S, ks, sigma):
    I, _ = planes(S, 3)
    rec = A.record(ks=ks, blur_sigma=sigma)
    k1 = rec["k1"][:ks]
    x = torch.linspace(-(ks - 1) * 0.5, (ks - 1) * 0.5, steps=ks)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    assert np.abs(k1 - (pdf / pdf.sum()).numpy()).max() <= 4 * U                # torchvision's kernel, to the last bit or two of exp
    assert abs(float(k1.astype(np.float64).sum()) - 1) <= ks * U
    oi, _ = A.stage_host("blur", I, None, rec)
    err = float(np.abs(oi - AC.torch_blur(I, k1)).max())
    # the same ks^2 products k1[y] k1[x] (one rounding each, alike on both sides) times values in [0, 1], weights summing to 1: only
    # the order of the n = ks^2 additions differs, n U a side
    bound = 2 * ks * ks * U
    print(f"blur S={S} ks={ks} sigma={sigma}: max |twin - conv2d| = {err:.3g} (bound {bound:.3g})")
    assert err <= bound


@pytest.mark.parametrize("S", AC.SIZES)
@pytest.mark.parametrize("f", [0.7, 1.3])
def test_brightness_and_contrast(S, f):
    I, _ = planes(S, 3)
    t = torch.from_numpy(I)
    oi, _ = A.stage_host("brightness", I, None, A.record(brightness=f))
    err = float(np.abs(oi - torch.clamp(t * f, 0.0, 1.0).numpy()).max())
    print(f"brightness S={S} f={f}: {err:.3g}")
    assert err <= 2 * U                                                       # one rounding of a product below 2, on each side
    oc, _ = A.stage_host("contrast", I, None, A.record(contrast=f))
    r = float(np.float32(f))
    t64 = t.double()
    ref = torch.clamp(r * t64 + (1.0 - r) * t64.mean(), 0.0, 1.0).numpy()     # `_blend(img, mean, ratio)` of adjust_contrast, in f64
    err = float(np.abs(oc - ref).max())
    # the twin's sum is 3 additions in a lane, 8 tree levels and at most S^2 / 1024 joins deep: depth d roundings, d U relative on a
    # mean <= 1, one more for the division; then (1 - r), two products and an addition of values below 2: 4 roundings of 2 U
    depth = 3 + 8 + -(-S * S // 1024) + 1
    bound = abs(1 - r) * depth * U + 4 * 2 * U
    print(f"contrast S={S} r={f}: max |twin - f64| = {err:.3g} (bound {bound:.3g})")
    assert err <= bound
    ref32 = torch.clamp(np.float32(f) * t + (1.0 - np.float32(f)) * t.mean(), 0.0, 1.0).numpy()
    assert float(np.abs(oc - ref32).max()) <= 2 * bound                       # and torch's own f32, as far from f64 as the twin may be


@pytest.mark.parametrize("S", AC.SIZES)
def test_an_off_stage_passes_its_input_through(S):
    I, M = planes(S, 1)
    off = A.record()
    for stage in ("rescale", "noise", "blur", "brightness", "contrast"):
        oi, om = A.stage_host(stage, I, M, off)
        assert np.array_equal(oi.view(np.uint32), I.view(np.uint32)) and np.array_equal(om, M), stage
    im, mk = AC.tiles(S)
    oi, om = A.augment_host(im, mk, [1, 0], augment=False)                    # the plain path: the validation loader
    assert np.array_equal(oi[:, 0], im[[1, 0]].astype(np.float32) / np.float32(255.0)) and np.array_equal(om[:, 0], (mk[[1, 0]] > 0).astype(np.float32))
    oi2, om2 = A.augment_host(im, mk, [1, 0], [off, off])                     # every stage off: the rotation by 0 is the identity
    assert np.array_equal(oi2, oi) and np.array_equal(om2, om)


@pytest.mark.parametrize("S", AC.SIZES)
def test_the_chain_is_the_composition_of_its_stages(S):
    im, mk = AC.tiles(S)
    for n, (cid, kw) in enumerate(AC.case_list(S)):
        rec = A.record(**kw)
        k = n % im.shape[0]
        I, M = im[k].astype(np.float32) / np.float32(255.0), (mk[k] > 0).astype(np.uint8)
        for stage in range(1, 8):
            I, M = A.stage_host(stage, I, M, rec)
        oi, om = A.augment_host(im, mk, [k], [rec])
        assert np.array_equal(oi[0, 0].view(np.uint32), I.view(np.uint32)) and np.array_equal(om[0, 0], M.astype(np.float32)), cid
        assert oi.min() >= 0 and oi.max() <= 1


def _normal_conditions(x):
    x = np.sort(np.asarray(x, np.float64))
    N = x.size
    cdf = 0.5 * (1 + np.array([math.erf(v / math.sqrt(2)) for v in x]))
    ks = max(np.max(np.arange(1, N + 1) / N - cdf), np.max(cdf - np.arange(N) / N))
    print(f"mean {x.mean():.4g} var {x.var():.5g} KS {ks:.4g} (limits {4 / math.sqrt(N):.4g}, {4 * math.sqrt(2 / N):.4g}, {1.63 / math.sqrt(N):.4g})")
    return abs(x.mean()) < 4 / math.sqrt(N) and abs(x.var() - 1) < 4 * math.sqrt(2 / N) and ks < 1.63 / math.sqrt(N)


def test_noise_is_standard_normal_and_a_function_of_key_and_index():
    N = 65536
    n = A.noise_host(AC.NOISE_KEY, N)
    assert n.dtype == np.float32 and np.isfinite(n).all()
    assert _normal_conditions(np.random.default_rng(AC.NOISE_KEY).standard_normal(N))      # the conditions hold for numpy's sample
    assert _normal_conditions(n)
    assert np.array_equal(n, A.noise_host(AC.NOISE_KEY, N)) and np.array_equal(n[:100], A.noise_host(AC.NOISE_KEY, 100))
    other = A.noise_host(AC.NOISE_KEY + 1, N)
    assert not np.array_equal(n, other) and abs(float(np.corrcoef(n, other)[0, 1])) < 4 / math.sqrt(N)
    S = 32
    I, _ = planes(S)
    rec = A.record(noise_sigma=0.05, noise_key=AC.NOISE_KEY)
    oi, _ = A.stage_host("noise", I, None, rec)
    assert np.array_equal(oi, np.clip(I + n[:S * S].reshape(S, S) * np.float32(0.05), 0, 1).astype(np.float32))


def reference_order(rng, S):
    """`_tensor_and_augment`'s draws, line by line (scripts/train_unet_crop.py:171-203)"""
    out = {"hflip": rng.random() > 0.5, "vflip": rng.random() > 0.5, "angle": rng.uniform(-30, 30), "new_size": 0, "sigma": 0.0, "ks": 0,
           "blur": None, "brightness": 0.0, "contrast": 0.0}
    if rng.random() > 0.5:
        out["new_size"] = int(S * rng.uniform(0.85, 1.15))
    if rng.random() > 0.5:
        out["sigma"] = rng.uniform(0.01, 0.05)
    if rng.random() > 0.5:
        out["ks"] = rng.choice([3, 5])
        out["blur"] = rng.uniform(0.5, 1.5)
    if rng.random() > 0.5:
        out["brightness"] = rng.uniform(0.7, 1.3)
    if rng.random() > 0.5:
        out["contrast"] = rng.uniform(0.7, 1.3)
    return out


def test_draw_consumes_the_generator_in_the_references_order():
    seen = set()
    for seed in range(1000):
        a, b = random.Random(seed), random.Random(seed)
        S = (32, 37, 256)[seed % 3]
        for _ in range(3):
            rec, want = A.draw(a, S, noise_key=seed), reference_order(b, S)
            t = math.radians(want["angle"])
            assert int(rec["flips"]) == int(want["hflip"]) + 2 * int(want["vflip"])
            assert rec["cos_t"] == np.float32(math.cos(t)) and rec["sin_t"] == np.float32(math.sin(t))
            assert int(rec["new_size"]) == want["new_size"] and rec["noise_sigma"] == np.float32(want["sigma"]) and int(rec["ks"]) == want["ks"]
            assert rec["brightness"] == np.float32(want["brightness"]) and rec["contrast"] == np.float32(want["contrast"])
            if want["ks"]:
                assert np.array_equal(rec["k1"][:want["ks"]], A.blur_kernel(want["ks"], want["blur"])) and not rec["k1"][want["ks"]:].any()
            else:
                assert not rec["k1"].any()
            assert int(rec["noise_key"]) == seed and int(rec["reserved"]) == 0
            seen.add((int(rec["flips"]), bool(rec["new_size"]), bool(rec["noise_sigma"]), int(rec["ks"]), bool(rec["brightness"]), bool(rec["contrast"])))
        assert a.getstate() == b.getstate(), seed                             # after N calls: the state of a reference-order consumer
    assert len(seen) > 150                                                    # (of 4 * 2 * 2 * 3 * 2 * 2 = 192 on / off patterns)
