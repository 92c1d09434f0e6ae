"""GPU (-m gpu): every layer tensor of every kernel form against a float64 reference of that one op, computed from the GPU's OWN
input tensor (oracle/layer_ref.py), at the precision the form's arithmetic reaches (kappa * 2^-24 * M per element).

The matrix (``layer_ref.GPU_CASES``) covers the canonical Winograd kernels at full and one-frame occupancy, the position-split
and wave-split forms, the direct kernels (occupancy, persistent, padded-channel), split K with the fused reduce and with the
separate epilogue, split precision, the fused first layer and fused head (checked by composition) and the unfused head, at frame
shapes where the tiles have edges.  Entry point: the u8 product path (``segment``).  The first ``nread`` frames of the (single)
chunk are read back: the special frames of ``layer_ref.special_frames`` (a mosaic of all-0 / all-255 / checkerboard / stripes
first, then random, all-0, all-255, checkerboard, stripes), the rest of the batch random.  The one-frame cases (nread 1) see
the mosaic only: its quadrants keep the four patterns pure in the shallow layers, but the deep layers of the 256 x 256 chains mix
them; the pure special frames are checked by the cases that read 3 or more frames (the 96 x 160, padded, 16 x 16 and five-level
nets).  Which kernels ran is asserted through
``UNet.profile`` here, and through ``og_unet_plan`` on the CPU (tests/test_layer_ref.py).

The f16 rows (``form`` "f16", precision 2) are judged by the interval test of ``layer_ref.check_f16``: every stored f16 value must
lie between the roundings of ``ref -+ kappa * 2^-24 * M``, a condition on its bits; their print line shows the smallest kappa each
layer needs.  ``test_f32_entry_point_in_f16_mode`` runs the same check on ``m(x)`` (NCHW floats in: ``k_conv_first_f<f32>``).

The f32 and split-precision rows cover every instantiation those two precisions can launch (``layer_ref.F32_KERNELS``, closed on
the CPU by tests/test_layer_ref.py), each on a shape with edges wherever the planner allows one; a row asserts the ``UNet.profile``
label of every kernel it claims.  That GPU assertion is weaker than the CPU one: ``UNet.profile`` gives ``OCC`` 3 and 4, ``SQ`` true
and false, split K with the fused reduce and with the epilogue, and a split and an unsplit ``k_conv_mfma_h`` / ``k_conv_mfma_p`` the
same label, so for those the evidence that the instantiation ran is that the row's plan (``og_unet_plan``, the product's own launch
decisions, claimed exactly on the CPU) is the chain the product runs.  ``test_f32_entry_point_in_f32_and_split_precision`` does for ``k_conv_first<float>`` /
``<float, true>`` what the f16 entry-point test does for its kernel.
"""
import numpy as np
import pytest

import openglottal_amd as og
from openglottal_amd import synth
from oracle import layer_ref as R

pytestmark = pytest.mark.gpu

ORDER = ["mosaic", "random", "zeros", "full", "checker", "stripes"]


def batch(H, W, B, seed=5):
    sp = R.special_frames(H, W, seed=seed)
    head = np.stack([sp[k] for k in ORDER])[:B]
    if B <= len(head):
        return np.ascontiguousarray(head)
    return np.concatenate([head, synth.random_gray_frames(B - len(head), H, W, seed=seed + 1)])


@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c["id"] for c in R.GPU_CASES])
def test_every_layer_against_float64(case):
    import torch

    feats, H, W, B, n = case["feats"], case["H"], case["W"], case["B"], case["nread"]
    sd = synth.make_unet_state_dict(feats, seed=11, head_scale=3.0, head_bias=-0.5)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    for k, v in case["options"].items():
        m.set_option(k, v)
    m.set_chunk(B)                    # one chunk: the activations read back are this batch's
    gray = batch(H, W, B)
    masks, areas, logits = m.segment(gray, want_logits=True)
    taps = {}

    def get(name):
        if name not in taps:
            taps[name] = m.activation(name, n)
        return taps[name]

    worst = R.check_net(sd, gray[:n], get, logits[:n], R.kappa_of(case["form"]), frames=[ORDER[i] if i < len(ORDER) else i for i in range(n)],
                        mask=masks[:n], area=areas[:n], fused_first=case["fused_first"], fused_head=case["fused_head"], form=case["form"])
    assert np.array_equal(areas, (masks > 0).reshape(B, -1).sum(1))
    prof = m.profile(torch.from_numpy(gray).cuda(), B, H, W, reps=1)
    if case["form"] == "f16":      # by the launch sites' whole labels, and nothing but f16-mode kernels
        labels = R.profile_instantiations(prof)
        assert set(case["prof"]) <= labels, (case["id"], sorted(set(case["prof"]) - labels), sorted(labels))
        assert all(k.startswith(("k_conv_mfma_f<", "k_conv_first_f<", "k_head_f", "k_sum_counts")) for k in labels), sorted(labels)
        layer = max(worst, key=worst.get)
        print(f"{case['id']} [f16 kappa {R.KAPPA['f16']:g}] smallest kappa each layer needs: "
              + " ".join(f"{k}={v:.2f}" for k, v in worst.items() if not k.startswith("pool")) + f"  (max {worst[layer]:.2f} at {layer})")
        return
    fams = R.profile_families(prof)
    assert set(case["prof"]) <= fams, (case["id"], sorted(set(case["prof"]) - fams), sorted(fams))
    labels = R.profile_instantiations(prof)    # and by instantiation: the labels of every kernel the row's plan claims (F32_KERNELS)
    assert case["prof_inst"] and set(case["prof_inst"]) <= labels, (case["id"], sorted(set(case["prof_inst"]) - labels), sorted(labels))
    print(f"{case['id']} [{case['form']} kappa {R.KAPPA[case['form']]:g}] worst |err|/bound per layer: "
          + " ".join(f"{k}={v:.3f}" for k, v in worst.items() if not k.startswith("pool")) + f"  (max {max(worst.values()):.3f})")


@pytest.mark.parametrize("feats", [(33, 66), R.FULL], ids=["padded-33x66", "full"])
def test_f32_entry_point_in_f16_mode(feats):
    """``m(x)``, NCHW floats in, in the f16 mode: the first layer is ``k_conv_first_f<f32>`` (the only first-layer kernel this entry
    point launches at precision 2).  The six special frames at 64 x 64 through the same per-layer interval check, and every tap and
    logit bit for bit what the u8 entry point (``segment``) gives for the same frames."""
    H = W = 64
    sd = synth.make_unet_state_dict(feats, seed=11, head_scale=3.0, head_bias=-0.5)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    m.set_option("precision", 2)
    gray = batch(H, W, len(ORDER))
    B = len(gray)
    m.set_chunk(B)
    logits = np.asarray(m((gray.astype(np.float32) / 255.0)[:, None]))[:, 0]
    taps = {name: m.activation(name, B) for name in R.layer_names(len(feats))}
    worst = R.check_net(sd, gray, taps.__getitem__, logits, R.kappa_of("f16"), frames=ORDER, form="f16")
    layer = max(worst, key=worst.get)
    print(f"f32 entry point {feats} [f16 kappa {R.KAPPA['f16']:g}] smallest kappa each layer needs: "
          + " ".join(f"{k}={v:.2f}" for k, v in worst.items() if not k.startswith("pool")) + f"  (max {worst[layer]:.2f} at {layer})")
    m.set_option("keep_taps", 1)
    _, _, lg_u8 = m.segment(gray, want_logits=True)
    assert np.array_equal(lg_u8, logits)
    for name, t in taps.items():
        assert np.array_equal(m.activation(name, B), t), name



@pytest.mark.parametrize("case", R.F32_ENTRY_CASES, ids=[c["id"] for c in R.F32_ENTRY_CASES])
def test_f32_entry_point_in_f32_and_split_precision(case):
    """``m(x)``, NCHW floats in, at precision 0 and 1: the first layer is ``k_conv_first<float>`` / ``<float, true>``, which the
    u8 product path never launches.  The six special frames at 64 x 64 through the per-layer check at the form's kappa, every tap
    and logit bit for bit what the u8 entry point (``segment``) gives for the same frames, and ``UNet.profile`` walking the float
    entry point's chain (option ``entry_f32``) names ``k_conv_first<f32>`` and the other kernels the case claims."""
    import torch

    feats, H, W = case["feats"], case["H"], case["W"]
    sd = synth.make_unet_state_dict(feats, seed=11, head_scale=3.0, head_bias=-0.5)
    m = og.UNet(1, 1, feats)
    m.load_state_dict(sd)
    m.to("cuda:0").eval()
    m.set_option("precision", case["options"]["precision"])
    gray = batch(H, W, len(ORDER))
    B = len(gray)
    assert B == case["B"]
    m.set_chunk(B)
    x = np.ascontiguousarray((gray.astype(np.float32) / 255.0)[:, None])
    logits = np.asarray(m(x))[:, 0]
    taps = {name: m.activation(name, B) for name in R.layer_names(len(feats))}
    worst = R.check_net(sd, gray, taps.__getitem__, logits, R.kappa_of(case["form"]), frames=ORDER, form=case["form"])
    print(f"{case['id']} [{case['form']} kappa {R.KAPPA[case['form']]:g}] worst |err|/bound per layer: "
          + " ".join(f"{k}={v:.3f}" for k, v in worst.items() if not k.startswith("pool")) + f"  (max {max(worst.values()):.3f})")
    m.set_option("keep_taps", 1)
    _, _, lg_u8 = m.segment(gray, want_logits=True)
    assert np.array_equal(lg_u8, logits)
    for name, t in taps.items():
        assert np.array_equal(m.activation(name, B), t), name
    m.set_option("entry_f32", 1)
    labels = R.profile_instantiations(m.profile(torch.from_numpy(x).cuda(), B, H, W, reps=1))
    assert "k_conv_first<f32>" in labels and "k_conv_first<u8>" not in labels, sorted(labels)
    assert set(case["prof_inst"]) <= labels, (case["id"], sorted(set(case["prof_inst"]) - labels), sorted(labels))
    with pytest.raises(og.OpenGlottalHipError, match="float32"):      # the option changes what profile reads: a u8 buffer is refused
        m.profile(torch.from_numpy(gray).cuda(), B, H, W, reps=1)
