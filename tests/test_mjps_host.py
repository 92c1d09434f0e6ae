"""The split entropy decoder's host twin (include/split/openglottal_hip_mjps.h) against the sequential twin: `decode_split_host` gives
`decode_host`'s pixels and status -- maximum difference 0 -- on Pillow files without DRI in every form, on two hostile corpora and on
hand-made gray scans, at subsequence lengths down to 4 bytes (shorter than one symbol with its value bits: pass-through lanes) and at
2 lanes per window (hundreds of windows); and on the files of the kernel's windows (tests/mjps_cases.py) with their firing checks, at
the kernel's own lanes per window.  No GPU."""
import numpy as np
import pytest

import mjpd_cases as DC
import mjps_cases as SC
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import OpenGlottalHipError

SIZES = ((1, 1), (8, 8), (17, 9), (37, 50), (64, 64))


@pytest.mark.parametrize("form", list(DC.FORMS))
@pytest.mark.parametrize("H,W", SIZES)
def test_pillow_files_without_dri_decode_as_the_sequential_twin_decodes_them(H, W, form):
    for quality in (1, 30, 75, 95, 100):
        for optimize in (False, True):
            j = DC.pillow_jpeg(H, W, form, quality, 0, optimize)
            assert MJ.parse(j)["Ri"] == 0
            assert SC.same_as_twin(j) == 0, (quality, optimize)


def test_quality_100_noise_puts_stuffed_pairs_on_lane_boundaries():
    j = DC.pillow_jpeg(64, 64, "444", 100, 0)
    lo, hi = DC.scan_span(j)
    pairs = [i - lo for i in range(lo, hi - 1) if j[i] == 0xFF and j[i + 1] == 0]
    assert any(p % 4 == 3 for p in pairs) and any(p % 4 == 0 for p in pairs)      # a lane of sub 4 starts on the 00, and on the FF
    assert SC.same_as_twin(j) == 0


def test_the_hostile_corpora_give_the_sequential_twin_s_statuses_and_pixels():
    seen = set()
    for label, b in SC.hostile():
        ref, st = DC.twin(b)
        for sub, lanes in SC.SMALL:
            out, st2 = SC.split(b, sub, lanes)
            assert st2 == st, (label, sub, lanes, st, st2)
            assert (out is None) if ref is None else np.array_equal(out, ref), (label, sub, lanes)
        seen.add(st)
    assert {0, 1, 2, 3, 6} <= seen


@pytest.mark.parametrize("name", ["dc-overflow", "dc-overflow-then-invalid", "invalid-then-dc-overflow", "zrl-overflow", "run-overflow", "intact",
                                  "garbage-before-eoi", "eoi-mid-scan", "app0-mid-scan", "rst-mid-scan"])
@pytest.mark.parametrize("H,W", [(8, 64), (37, 50)])
def test_hand_made_scans(H, W, name):
    j, claim = SC.handmade(H, W)[name]
    assert DC.twin(j)[1] == claim                                             # the sequential twin confirms the case
    assert SC.same_as_twin(j) == claim
    if name == "dc-overflow":                                                 # blocks 0 and 1 are written, nothing from block 2 on
        f = DC.twin(j)[0]
        assert np.all(f[:8, :16] == 255) and np.all(f[:8, 16:] == 128) and np.all(f[8:] == 128)


def test_stats_rounds_stay_within_the_lanes_and_lane_0_decodes_once_per_window():
    j = DC.pillow_jpeg(64, 64, "444", 95, 0)
    n = MJ.parse(j)["scan_length"]
    for sub, lanes in SC.PAIRS + ((32, 256), (128, 7)):
        per = min(lanes, MJ.split_limit(4) // sub)
        _, st, s = SC.split(j, sub, lanes, stats=True)
        assert st == 0 and 1 <= s["rounds"] <= per
        # (the data ends at EOI, the scan's length; a last window that only holds the padding behind the last MCU is not walked)
        assert -(-n // sub) - 1 <= s["lanes"] <= -(-n // sub)
        assert s["windows"] == -(-s["lanes"] // per)
        assert s["lanes"] <= s["decodes"] <= s["lanes"] * per
    # one lane per window: its entry is exact and never changes, so every window decodes exactly once, in one round
    _, st, s = SC.split(j, 64, 1, stats=True)
    assert st == 0 and s["rounds"] == 1 and s["decodes"] == s["windows"] == s["lanes"]
    # lane 0 of a window never decodes twice: with two lanes per window at most the second lane repeats, once
    _, st, s = SC.split(j, 64, 2, stats=True)
    assert s["decodes"] <= s["lanes"] + s["windows"] and s["rounds"] <= 2
    # a file with restart markers is decoded as before and counts nothing
    r = DC.pillow_jpeg(17, 9, "420", 75, 1)
    out, st, s = SC.split(r, 4, 256, stats=True)
    assert st == 0 and np.array_equal(out, DC.twin(r)[0]) and s == {"lanes": 0, "windows": 0, "rounds": 0, "decodes": 0}


# ── the files of the kernel's windows (tests/test_gpu_mjps.py decodes the same cached files on the device) ──────────────────────────
@pytest.mark.parametrize("group", SC.GROUPS)
def test_the_window_files_decode_as_the_sequential_twin_decodes_them(group):
    """Every file built for the window tests, at PAIRS and at sub 256, 512 and 128; a file above 32 KB keeps 256 lanes, so that the
    twin walks the kernel's real windows.  The Pillow files are held to Pillow once."""
    for label, j in SC.group(group):
        assert SC.same_as_twin(j, SC.pairs_for(j)) == DC.twin(j)[1], label
        if group in ("real", "mixed") and DC.twin(j)[1] == 0:
            assert np.array_equal(DC.twin(j)[0], DC.pillow_bgr(j)), label


@pytest.mark.parametrize("name", list(SC.REAL))
def test_real_windows_fire(name):
    SC.real_fires(name)


@pytest.mark.parametrize("sub", [4, 8])
def test_the_placed_bytes_fire(sub):
    for name in SC.EDGES:
        SC.edge_fires(name, sub)
    for name in SC.ENDS:
        SC.end_fires(name, sub)
        SC.cut_fires(name, sub)
    SC.symbol_edge_fires(sub)


@pytest.mark.parametrize("sub", [4, 8])
def test_the_late_errors_fire(sub):
    for name in SC.late_errors(sub):
        SC.late_fires(name, sub)
    # the overflow is the third of three + 1000 steps; the twin's frame shows the two before it written and nothing behind them
    j, _, at = SC.late_errors(sub)["dc-overflow-in-window-1"]
    ok, _, _ = SC.late_errors(sub)["intact"]
    assert not np.array_equal(DC.twin(j)[0], DC.twin(ok)[0]) and (DC.twin(j)[0][-8:] == 128).all()


def test_the_mixed_batch_fires():
    for sub in (256, 4):
        SC.mixed_fires(sub)


def test_the_hand_made_scan_of_three_windows_at_sub_1024_is_written_quickly_enough():
    """The case is kept because the Python writer takes under 2 s for its 77 KB (0.2 s on an idle machine where this was written, 1.5 s
    beside a compiler run); the time is printed, not asserted."""
    j = SC.three_windows_at_1024()
    print(f"three_windows_at_1024: {len(j)} bytes written in {SC.BUILD_SECONDS['three-windows-at-1024']:.2f} s")
    _, st, stats = SC.kernel_twin(j, 1024)
    assert st == DC.twin(j)[1] == 0 and stats["windows"] >= 3 and MJ.parse(j)["scan_length"] > 2 * SC.WINDOW


def test_rounds_over_the_window_files_stay_within_the_lanes_of_a_window():
    """The header's bound, rounds <= lanes of the window, over every file above at the kernel's lanes; the largest per sub is printed
    (DESIGN section 24 quotes it)."""
    for sub in (4, 8, 64, 128, 256, 512, 1024):
        worst = (0, None)
        for group in SC.GROUPS:
            for label, j in SC.group(group):
                rounds = SC.kernel_twin(j, sub)[2]["rounds"]
                assert rounds <= SC.lanes_of(sub), (sub, group, label)
                worst = max(worst, (rounds, f"{group}/{label}"))
        print(f"sub {sub}: {SC.lanes_of(sub)} lanes a window, at most {worst[0]} rounds ({worst[1]})")


def test_the_twin_refuses_bad_arguments_and_the_defaults_are_the_limits():
    j = DC.pillow_jpeg(8, 8, "444")
    assert [MJ.split_limit(i) for i in (1, 2, 3, 4)] == [4, 1024, 256, 32768] and MJ.split_limit(0) % 4 == 0
    assert 4 <= MJ.split_limit(0) <= 1024 and 0 < MJ.split_limit(5) <= 65536 and MJ.split_limit(6) == -1 and MJ.split_limit(-1) == -1
    for sub, lanes in ((2, 4), (6, 4), (1028, 4), (-4, 4), (4, 0), (4, 257)):
        with pytest.raises(OpenGlottalHipError):
            MJ.decode_split_host(j, sub, lanes)
    assert np.array_equal(MJ.decode_split_host(j), DC.twin(j)[0])            # sub 0: the default
    with pytest.raises(OpenGlottalHipError):
        MJ.decode_split_host(b"junk", 4, 4)
    assert MJ.decode_split_host(b"junk", 4, 4, statuses=True) == (None, 6)
