"""CPU: the f16 inference mode (`precision=2`) without a GPU.

* the launch decisions of an f16 chain (og_unet_plan / og_unet_plan_resized): every launch inside the library's limits, every conv
  launch a k_conv_mfma_f one, no more launches than split precision plans for the same call, the arena at most 0.6 x the f32 one
  (2 instead of 4 bytes per channel);
* `precision=3` is still an error; "splitk" 1 and "precision" 2 exclude each other (the mode never splits K);
* the CPU emulation the GPU tests judge the kernels by (tests/f16_emulation.py), alone: its f32 path reproduces the reference
  fixtures' masks exactly (this pins the emulation to the reference), and its f16 path is run in both memory formats -- E (error
  against the reference) and D (difference between the two summation orders) are printed.
"""
import ctypes as C
import os

import numpy as np
import pytest

import f16_emulation as EMU
from openglottal_amd import synth
from openglottal_amd._lib import lib
from test_launch_plan import FULL, check, plan
from test_resize_host import plan_resized

def is_conv(kernel):
    return "k_conv" in kernel and "k_conv_first" not in kernel


def check_f16_chain(recs, what):
    check(recs, what)
    convs = [r["kernel"] for r in recs if is_conv(r["kernel"])]
    assert convs and all(k.startswith("(k_conv_mfma_f<") for k in convs), (what, convs)
    assert sum(r["ws"] for r in recs) == 0 and sum(r["cnt"] for r in recs) == 0, what     # no split-K workspace in this mode


def test_every_micro_batch_size_of_the_full_width_net_in_f16_mode():
    for B in list(range(1, 65)) + [96, 128, 256]:
        for lanes in (1, 3):
            recs, arena2 = plan(FULL, B, 256, 256, lanes, "precision=2")
            check_f16_chain(recs, (B, lanes))
            recs1, _ = plan(FULL, B, 256, 256, lanes, "precision=1")
            assert len(recs) <= len(recs1), (B, lanes, len(recs), len(recs1))
            _, arena0 = plan(FULL, B, 256, 256, lanes, "")
            assert arena2 <= 0.6 * arena0, (B, arena2, arena0)
    r1, _ = plan(FULL, 1, 256, 256, 1, "precision=2")
    r64, _ = plan(FULL, 64, 256, 256, 2, "precision=2")
    assert len(r1) <= 23 and len(r64) <= 22, (len(r1), len(r64))
    assert r1[0]["kernel"].startswith("k_conv_first_f") and r64[0]["kernel"].startswith("(k_conv_mfma_f<1, 0, 8, 3, true>")
    # 17 3x3 convs + 4 transposed convs: all of them on the f16 kernel
    assert sum(is_conv(r["kernel"]) for r in r1) == 21 and sum(is_conv(r["kernel"]) for r in r64) == 21


@pytest.mark.parametrize("feats,shape", [((32, 64), (128, 256)), ((32, 64), (96, 160)), ((64, 128), (48, 64)), ((40, 80), (64, 64)),
                                         ((32, 64, 128), (64, 32)), ((4, 8, 16, 32), (256, 256)), ((32, 64, 128, 256), (512, 512)),
                                         ((16, 32, 64, 128, 256), (256, 256)), ((96, 192), (64, 128)),
                                         ((32, 64, 128), (80, 48)), ((33, 66), (32, 64)), ((6, 12, 24), (48, 32))])
def test_other_nets_and_frame_shapes_in_f16_mode(feats, shape):
    H, W = shape
    for options in ("precision=2", "precision=2,fuse_head=0", "precision=2,fuse_first=0", "precision=2,tile_h=8", "precision=2,h_square=0"):
        for B in (1, 2, 3, 5, 11, 16, 33, 64):
            recs, arena2 = plan(feats, B, H, W, 1, options)
            check_f16_chain(recs, (feats, shape, options, B))
            recs1, _ = plan(feats, B, H, W, 1, options.replace("precision=2", "precision=1"))
            assert len(recs) <= len(recs1), (feats, shape, options, B)
            _, arena0 = plan(feats, B, H, W, 1, "")
            assert arena2 <= 0.6 * arena0, (feats, shape, B, arena2, arena0)


def test_bad_precision_values_and_split_k_are_refused():
    l = lib()
    buf = C.create_string_buffer(1 << 16)
    f = (C.c_int * 4)(*FULL)
    assert l.og_unet_plan(f, 4, 1, 256, 256, 1, b"precision=3", buf, len(buf), None) == -1
    assert "precision" in l.og_last_error().decode()
    assert l.og_unet_plan(f, 4, 1, 256, 256, 1, b"precision=-1", buf, len(buf), None) == -1
    assert l.og_unet_plan(f, 4, 1, 256, 256, 1, b"precision=2,splitk=1", buf, len(buf), None) == -1
    assert l.og_unet_plan(f, 4, 1, 256, 256, 1, b"splitk=1,precision=2", buf, len(buf), None) == -1
    assert l.og_unet_plan(f, 4, 1, 256, 256, 1, b"precision=2", buf, len(buf), None) > 0


@pytest.mark.parametrize("H,W", [(512, 512), (480, 640), (200, 100), (255, 257), (1080, 1920)])
def test_resized_plan_in_f16_mode_stays_inside_limits_and_caller_buffers(H, W):
    l = lib()
    ws_max, cnt_max, g_max, lds_max = (l.og_workspace_limit(i) for i in range(4))
    for ch in (1, 3):
        for B in (1, 2, 7, 31, 32, 33, 64):
            n, recs = plan_resized(B, H, W, ch, options="precision=2")
            assert n > 0, (H, W, ch, B, l.og_last_error())
            limit = {"mask": B * H * W, "area": 4 * B, "net_logits": 4 * B * 256 * 256, "net_prob": 4 * B * 256 * 256, "prob": 4 * B * H * W}
            seen = {k: 0 for k in limit}
            for r in recs:
                gx, gy, gz = r["grid"]
                assert gx >= 1 and gy >= 1 and gz >= 1 and gy <= g_max and gz <= g_max and gx < 2 ** 31, (H, W, B, r)
                assert r["block"] == 256 and r["lds"] <= lds_max and r["ws"] <= ws_max and r["cnt"] <= cnt_max, (H, W, B, r)
                for k, end in r["writes"].items():
                    assert 0 < end <= limit[k], (H, W, ch, B, r)
                    seen[k] = max(seen[k], end)
            assert seen == limit, (H, W, ch, B, seen)
            convs = [r["kernel"] for r in recs if is_conv(r["kernel"])]
            assert convs and all(k.startswith("(k_conv_mfma_f<") for k in convs), convs


def _unpack(bits, n):
    return np.unpackbits(bits, axis=1)[:, :65536].reshape(n, 256, 256)


def test_the_emulation_is_pinned_to_the_reference_fixtures(golden_dir):
    """f32 path of the emulation == the fixtures' masks, every pixel; then E and D of the f16 path (printed: the GPU tests compute
    them again on the frames they run)."""
    g = np.load(os.path.join(golden_dir, "unet_trained_small.npz"))
    sd = {k[2:]: g[k] for k in g.files if k.startswith("W:")}
    frames, _ = synth.glottis_frames(4, 20, seed=99)
    frames = frames[:16]
    ref = EMU.logits(sd, frames, half=False)
    assert np.array_equal(EMU.masks_from_logits(ref), _unpack(g["masks_packed"][:16], 16) > 0)
    ref_cl = EMU.logits(sd, frames, half=False, channels_last=True)
    E, D, a, b = EMU.emulation_error(sd, frames, ref)
    print(f"unet_trained_small[:16]: E {E:.3g}  D {D:.3g}  f32 order noise {np.abs(ref - ref_cl).max():.3g}  max|logit| {np.abs(ref).max():.3g}")
    assert 0 < E < 0.1 * np.abs(ref).max() and np.isfinite(a).all() and np.isfinite(b).all()     # the rounding is there, and it is small

    gh = np.load(os.path.join(golden_dir, "unet_trained_hard.npz"))
    g9 = np.load(os.path.join(golden_dir, "unet_trained_full.npz"))
    sdh = synth.detuned_weights({k[2:]: g9[k] for k in g9.files if k.startswith("W:")})
    clean, _ = synth.glottis_frames(4, 20, seed=99)
    hard, _ = synth.degraded_glottis_frames()
    allf = np.concatenate([clean, hard])
    idx = np.r_[0:8, 80:88]          # 8 clean + 8 degraded frames
    refh = EMU.logits(sdh, allf[idx], half=False)
    m_ref = _unpack(gh["masks_packed"][idx], 16) > 0
    diff = EMU.masks_from_logits(refh) != m_ref
    # the hard fixture has logits down to 3.6e-7: the oracle may differ from the reference only inside the reference's own noise band
    import oracle
    assert np.all(np.abs(refh[diff]) <= oracle.reference_band()), np.abs(refh[diff]).max()
    Eh, Dh, _, _ = EMU.emulation_error(sdh, allf[idx], refh)
    print(f"unet_trained_hard[16]: E {Eh:.3g}  D {Dh:.3g}  max|logit| {np.abs(refh).max():.3g}  oracle-vs-fixture flips {int(diff.sum())}")
    assert 0 < Eh < 0.1 * np.abs(refh).max()


def test_emulation_layer_taps_cover_the_small_layer_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "unet_small_layers.npz"))
    sd = synth.make_unet_state_dict(tuple(g["features"]), seed=int(g["seed"]), head_scale=float(g["head_scale"]), head_bias=float(g["head_bias"]))
    x = (synth.random_gray_frames(1, 64, 64, seed=21).astype("float32") / 255.0)[:, None]
    keys = [k[2:] for k in g.files if k.startswith("L:")]
    assert len(keys) == 27
    t32 = EMU.layer_taps(sd, x, half=False)
    t16 = EMU.layer_taps(sd, x, half=True)
    t16c = EMU.layer_taps(sd, x, half=True, channels_last=True)
    import oracle
    band = oracle.reference_band()
    for k in keys:
        ref = g["L:" + k]
        assert t32[k].shape == ref.shape == t16[k].shape == t16c[k].shape, k
        assert np.abs(t32[k] - ref).max() <= band * max(1.0, np.abs(ref).max()), k      # f32 path: the reference's tensors
        e = max(np.abs(t16[k] - ref).max(), np.abs(t16c[k] - ref).max())
        assert e > 0, k                                                                  # every tensor is rounded
        if k != "head":
            assert np.array_equal(t16[k], t16[k].astype(np.float16).astype(np.float32)), k   # stored values are f16 values
