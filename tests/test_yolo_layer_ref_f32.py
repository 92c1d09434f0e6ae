"""CPU: the float64 per-launch reference of the f32 detector (oracle/yolo_layer_ref.py: ``check_launch_f32``) judged on its own, and
the list of kernels the f32 detector can launch (``YOLO_F32_KERNELS``) closed against ``og_yolo_plan`` at 256 CUs.

* a torch-f32 CPU emulation of every launch passes at kappa 16, NCHW and channels_last, on the ``n`` net and on the 0.375 / 0.67 net;
  the kappa it needs is recorded as ``YOLO_F32_EMULATED_MAX`` (asserted within 2x);
* eleven wrong ways to run ONE launch are each flagged at that launch; the ratio of the weakest is printed;
* the launch references chained from the input restate ``yolo_oracle.forward`` (the pin ``full_forward`` has for modules);
* the option sweep shows no instantiation outside the list, every entry is reached by its own case, the GPU rows
  (``GPU_ROWS``, tests/test_gpu_yolo_launch_parity.py) run every entry on a shape with partial tiles, and the rows that cover no
  entry alone are exactly the listed ones.
"""
import itertools

import numpy as np
import pytest

from openglottal_amd import synth
from oracle import layer_ref as LR
from oracle import yolo_layer_ref as YR
from oracle import yolo_oracle as Y

N_CU = 256
_sd = {}


def net(name):
    if name not in _sd:
        _sd[name] = synth.make_yolov8_state_dict(**YR.NETS[name])
    return _sd[name]


def input_of(H, W, B=1, seed=3):
    return Y.preprocess_bgr(np.random.RandomState(seed).randint(0, 256, (B, H, W, 3), dtype=np.uint8)).numpy()


# ───────────────────────────── the emulation passes ─────────────────────────────


@pytest.mark.parametrize("shape", [(96, 160), (32, 32), (160, 256), (480, 512)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", ["n", "w375"])
def test_f32_emulation_passes_every_launch_at_kappa_16(name, shape):
    sd, x = net(name), input_of(*shape)
    top = {}
    for cl in (False, True):
        taps = YR.emulate_f32(sd, x, channels_last=cl)
        need = {s["name"]: YR.check_launch_f32(s, sd, taps) for s in YR.launches(sd)}
        k = max(need, key=need.get)
        top[cl] = (need[k], k)
    print(f"{name} {shape[0]}x{shape[1]}: largest kappa needed NCHW {top[False][0]:.2f} ({top[False][1]}), "
          f"channels_last {top[True][0]:.2f} ({top[True][1]}) of {YR.KAPPA['direct']:g}")
    worst = max(v[0] for v in top.values())
    assert worst <= YR.KAPPA["direct"]
    assert worst <= 2 * YR.YOLO_F32_EMULATED_MAX, worst


# ───────────────────────────── planted single-launch mutants ─────────────────────────────

# mutant -> the launch it is planted in, on the wider net at 160 x 256 (a 5 x 8 deepest map: the chained pools differ from one another)
TARGETS = {
    "bn_eps_1e5": "model.4.cv1",
    "last_chunk_dropped": "model.6.cv2",          # 6 segments of 48 channels: the last padded chunk is half of m.3.cv2
    "k_part_dropped": "model.8.m.0.cv1",
    "s2_taps_swapped": "model.5",
    "res_wrong_half": "model.4.m.0.cv2",
    "head_zero_block_filled": "model.22.cv2.1.1",
    "pool_wrong_segment": "model.9.m.2",
    "up_shifted": "model.10",
    "operands_10bit": "model.12.cv1",
    "weights_f16": "model.15.m.0.cv1",
    "silu_of_f16": "model.18.cv1",
}
_ratios = {}


@pytest.fixture(scope="module")
def emu():
    sd = net("w375")
    return sd, YR.emulate_f32(sd, input_of(160, 256, B=2))


def test_every_mutant_has_a_target():
    assert set(TARGETS) == set(YR.MUTANTS_F32)


def plant(emu, mut):
    """Run TARGETS[mut] the wrong way; -> (launch name, worst |err| / bound, elements over) once the check has flagged it there."""
    if mut in _ratios:
        return _ratios[mut]
    sd, good = emu
    spec = next(s for s in YR.launches(sd) if s["name"] == TARGETS[mut])
    taps = dict(good)
    bad = YR.emu_launch_f32(spec, sd, taps, mut=mut)
    assert bad.shape == good[spec["name"]].shape and not np.array_equal(bad, good[spec["name"]]), f"{mut} changes nothing in {spec['name']}"
    YR.check_launch_f32(spec, sd, taps)          # the right launch passes
    taps[spec["name"]] = bad
    with pytest.raises(LR.LayerMismatch) as ei:
        YR.check_launch_f32(spec, sd, taps)
    assert str(ei.value).startswith(spec["name"] + ":"), str(ei.value)
    ref, e = YR.ref_launch_f32(spec, sd, taps)
    if e is None:
        ratio, over = float("inf"), int((bad != ref).sum())
    else:
        r = np.abs(bad.astype(np.float64) - ref) / e
        ratio, over = float(r.max()), int((r > 1).sum())
    _ratios[mut] = (spec["name"], ratio, over)
    return _ratios[mut]


@pytest.mark.parametrize("mut", YR.MUTANTS_F32)
def test_planted_mutant_is_flagged_at_its_launch(emu, mut):
    name, ratio, over = plant(emu, mut)
    print(f"{mut} at {name}: worst |err| / bound {ratio:.3g}, {over} element(s) over")
    assert over >= 1 and ratio > 1.0


def test_weakest_mutant_is_still_over_the_bound(emu):
    got = {m: plant(emu, m) for m in YR.MUTANTS_F32}
    weakest = min(got, key=lambda m: got[m][1])
    print(f"weakest mutant: {weakest} at {got[weakest][0]}, |err| / bound = {got[weakest][1]:.3g}")
    assert got[weakest][1] > 1.0


# ───────────────────────────── restatement pin ─────────────────────────────


def test_chained_launch_references_restate_the_oracle():
    """The launch references chained from the preprocessed input (float64 values, the device's f32 scale and shift) stay within the
    module chain's propagated bound of ``full_forward`` -- which tests/test_yolo_layer_ref.py pins to ``yolo_oracle.forward`` -- and
    the f32 oracle's own taps stay within that bound of them."""
    import torch

    sd = net("n")
    x = input_of(64, 96, B=2)
    chain = YR.chain_refs(sd, x)
    mods = YR.full_forward(sd, x)
    with torch.no_grad():
        _, oracle = Y.forward(sd, torch.from_numpy(x))
    name_of = {n: (n if n + ".cv2.conv.weight" not in sd else n + ".cv2") for n in YR.MODULES if n.startswith("model.")}
    name_of["model.9"] = "model.9.cv2"
    for l in range(3):
        name_of[f"box{l}"], name_of[f"cls{l}"] = f"model.22.cv2.{l}.2", f"model.22.cv3.{l}.2"
    assert set(name_of) == set(YR.MODULES)
    for n, tap in name_of.items():
        YR.check_module(n, chain[tap], mods[n])
        r, e = mods[n].v.numpy(), mods[n].e.numpy() + 1e-30
        assert np.all(np.abs(oracle[n].numpy().astype(np.float64) - chain[tap]) <= 2 * e), n
    assert set(chain) - {"input"} == set(YR.tap_names(sd))


def test_f16_reference_still_sees_the_same_chain():
    import yolo_f16_ref as R

    assert R.launches is YR.launches and R.tap_names is YR.tap_names and R.gather is YR.gather and R.affine is YR.affine


# ───────────────────────────── og_yolo_plan and the closed list ─────────────────────────────

SWEEP_NETS = ("n", "w375", "w125")
SWEEP_SHAPES = ((32, 32), (96, 160), (160, 256), (224, 352), (256, 256), (384, 384), (480, 512))
SWEEP_BATCHES = (1, 2, 3, 48, 64, 192)
SWEEP_OPTIONS = dict(latency_batch=(0, 1, 4, 64), latency_nt1=(0, 1), head_fused=(0, 1), splitk_max=(1, 2, 8, 64), splitk_min_steps=(1, 3, 9),
                     splitk_slots=(1, 4), splitk_div=(1, 2, 8))
_planners, _sweep_cache = {}, {}


def planner(name):
    from openglottal_amd.yolo import YoloPlanner

    if name not in _planners:
        _planners[name] = YoloPlanner(net(name))
    return _planners[name]


def plan_of(name, H, W, B, options):
    return planner(name).plan(B, H, W, N_CU, options)


def _sweep_part(args):
    from openglottal_amd.yolo import YoloPlanner

    name, shape = args
    P = YoloPlanner(net(name))
    option_sets = [",".join(f"{k}={v}" for k, v in zip(SWEEP_OPTIONS, vs)) for vs in itertools.product(*SWEEP_OPTIONS.values())]
    raw, texts = {}, set()
    for B in SWEEP_BATCHES:
        for o in option_sets:
            txt = P.plan_text(B, shape[0], shape[1], N_CU, o, want_arena=False)
            if txt in texts:   # (most option sets change nothing for a given shape and batch)
                continue
            texts.add(txt)
            for line in txt.splitlines():
                f = line.split("|")
                part = "mfma" not in f[0] or YR.has_partial_tile(dict(module=f[8]), *shape)
                raw.setdefault((f[0], part), (name, shape[0], shape[1], B, o))
    return raw


def sweep():
    """{(instantiation, on a launch with a partial tile): a (net, H, W, B, options) that shows it} over the whole cross product."""
    if not _sweep_cache:
        for n in SWEEP_NETS:
            for shape in SWEEP_SHAPES:
                for (k, part), where in _sweep_part((n, shape)).items():
                    _sweep_cache.setdefault((YR.plan_labels([(k, "")])[0], part), where)
    return _sweep_cache


def matrix_cover():
    """({instantiation: [row ids]}, the same over the rows where a launch of it has a partial tile) from the PLANS of GPU_ROWS."""
    every, edges = {}, {}
    for r in YR.GPU_ROWS:
        recs = plan_of(r["net"], r["H"], r["W"], r["B"], r["options"])
        for lab, rec in zip(YR.plan_labels(recs), recs):
            if r["id"] not in every.setdefault(lab, []):
                every[lab].append(r["id"])
            if ("mfma" not in lab or YR.has_partial_tile(rec, r["H"], r["W"])) and r["id"] not in edges.setdefault(lab, []):
                edges[lab].append(r["id"])
    return every, edges


def test_plan_runs_without_a_device_and_names_every_launch():
    recs = plan_of("n", 256, 256, 1, "")
    assert len(recs) == 58 and planner("n").arena_bytes > 0
    assert recs[0]["kernel"] == "k_conv_direct<true, 1> cq_shift=2" and recs[0]["module"] == "model.0"
    assert recs[1]["kernel"] == "k_conv_mfma_o<1, 3, 8, 3, false, false> ksplit=4" and recs[1]["ws"] > 0 and recs[1]["cnt"] == 32
    assert recs[-1]["kernel"] == "k_yolo_decode_mb" and recs[-1]["module"] == "model.22"
    mods = [r["module"] for r in recs]
    assert "model.9.m.1-3" in mods and "model.22.hd.0.1" in mods and "model.10" in mods
    two = plan_of("n", 256, 256, 2, "")
    assert two[1]["kernel"] == "k_conv_mfma_o<1, 3, 8, 3, false, true> vsplit=4" and two[1]["ws"] == 0
    assert [r["module"] for r in two if r["kernel"] == "k_maxpool5"] == ["model.9.m.1", "model.9.m.2", "model.9.m.3"]
    # every template argument resolved: no launch-site text survives
    for r in recs + two + plan_of("n", 96, 160, 2, "precision=2"):
        assert "NT" not in r["kernel"] and "MODE" not in r["kernel"] and "(" not in r["kernel"], r["kernel"]
        assert r["module"].startswith("model."), r
    # the CU count is the caller's
    assert [r["kernel"] for r in planner("n").plan(48, 96, 160, 64, "")] != [r["kernel"] for r in planner("n").plan(48, 96, 160, 256, "")]


def test_plan_refuses_bad_arguments_and_finalized_handles():
    from openglottal_amd._lib import OpenGlottalHipError

    P = planner("n")
    for args in ((0, 256, 256, 0, ""), (1, 250, 256, 0, ""), (1, 256, 256, -1, ""), (1, 256, 256, 0, "splitk_max=0"), (1, 256, 256, 0, "nonsense=1"),
                 (1, 256, 256, 0, "splitk_max")):
        with pytest.raises(OpenGlottalHipError):
            P.plan_text(*args)
    assert len(P.plan(1, 256, 256, 0, "")) == 58   # the handle stays usable, and its options are its own again
    # the text is bounded by cap: a buffer one byte short is refused and left alone, one that fits exactly is filled
    import ctypes as C
    from openglottal_amd._lib import lib

    need = len(P.plan_text(1, 256, 256, 0, "").encode()) + 1
    small = C.create_string_buffer(b"\x7f" * need, need + 8)
    assert lib().og_yolo_plan(P._h, 1, 256, 256, 0, b"", small, need - 1, None) < 0 and small.raw[:need] == b"\x7f" * need
    assert lib().og_yolo_plan(P._h, 1, 256, 256, 0, b"", small, need, None) == 58 and small.raw[need:] == b"\x00" * 8
    assert lib().og_yolo_last_launches(P._h, small, need) == 0 and small.raw[:1] == b"\x00"   # (no chain has run on this handle)
    assert lib().og_yolo_last_launches(P._h, small, 0) < 0 and lib().og_yolo_last_launches(None, small, need) < 0
    from openglottal_amd.yolo import YoloPlanner

    with pytest.raises(OpenGlottalHipError, match="bottleneck|incomplete|missing"):
        YoloPlanner({k: v for k, v in net("n").items() if not k.startswith("model.8.")}).plan_text(1, 256, 256, 0, "")


def test_f32_kernel_list_is_closed_under_the_option_sweep():
    texts = {v[0] for v in YR.YOLO_F32_KERNELS.values()}
    assert len(texts) == len(YR.YOLO_F32_KERNELS) == 29
    seen = sweep()
    unknown = {k: w for (k, _), w in seen.items() if k not in texts}
    assert not unknown, ("instantiations the list does not know, and a plan that shows each", unknown)
    assert texts == {k for k, _ in seen}, sorted(texts - {k for k, _ in seen})   # nothing unreachable stays listed
    for short, (text, (name, H, W, B, options)) in YR.YOLO_F32_KERNELS.items():
        recs = plan_of(name, H, W, B, options)
        hit = [r for lab, r in zip(YR.plan_labels(recs), recs) if lab == text]
        assert hit, (short, text, "is not reached by", (name, H, W, B, options))
        assert "mfma" not in text or any(YR.has_partial_tile(r, H, W) for r in hit), (short, "its own case has no partial tile")


def test_gpu_rows_run_every_listed_instantiation_on_a_partial_tile():
    every, edges = matrix_cover()
    texts = {v[0] for v in YR.YOLO_F32_KERNELS.values()}
    assert set(every) == texts, ("never compared with float64:", sorted(texts - set(every)), "unlisted:", sorted(set(every) - texts))
    on_edges = {k for (k, part) in sweep() if part}
    for text, rule in YR.YOLO_EDGE_EXEMPT.items():
        assert text not in on_edges and rule, (text, "is exempt but reachable with a partial tile")
    lost = on_edges - set(edges)
    assert not lost, ("reachable with a partial tile but judged on none", sorted(lost))
    assert len({r["id"] for r in YR.GPU_ROWS}) == len(YR.GPU_ROWS)


def test_rows_redundant_for_coverage_are_exactly_the_listed_ones():
    every, edges = matrix_cover()
    sole = {rows[0] for rows in list(every.values()) + list(edges.values()) if len(rows) == 1}
    redundant = {r["id"] for r in YR.GPU_ROWS} - sole
    listed = set(YR.YOLO_REDUNDANT_FOR_COVERAGE)
    assert redundant == listed, (sorted(redundant - listed), sorted(listed - redundant))
    assert all(YR.YOLO_REDUNDANT_FOR_COVERAGE.values())


def test_wider_net_has_the_shapes_the_n_net_lacks():
    """At 0.375 / 0.67: 24/48/96/192/384 channels, up to 4 bottlenecks, and a stacked head of 160 padded channels (NT = 1, 5 column tiles)."""
    sd = net("w375")
    assert [sd[f"model.{i}.conv.weight"].shape[0] for i in (0, 1, 3, 5, 7)] == [24, 48, 96, 192, 384]
    assert max(j for j in range(8) if f"model.6.m.{j}.cv1.conv.weight" in sd) == 3
    recs = plan_of("w375", 96, 160, 1, "")
    hd = next(r for r in recs if r["module"] == "model.22.hd.0.1")
    assert hd["kernel"].startswith("k_conv_mfma_o<1, 0, 8, 3, false, false> ksplit=") and hd["gz"] % 5 == 0, hd
