"""-m gpu: k_mjps_entropy (include/split/openglottal_hip_mjps.h), the split entropy pass of files without restart markers.  Device bytes
and statuses = the split twin's = the sequential twin's = the same handle's with the mode off, in the smallest shapes where each
mechanism can go wrong: several windows at sub 4, every form, damaged frames beside an intact one under guard zones; and the window
machinery that only the kernel has (staging, data-end search, lane masks) on real windows at every sub, on bytes placed at window
edges, on errors behind window 0 and at the four source alignments."""
import numpy as np
import pytest
import torch

import buffer_guard as G
import mjpd_cases as DC
import mjps_cases as SC
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import lib

pytestmark = pytest.mark.gpu


def _resident(d, files):
    blob, offsets, recs, tabs, form = MJ.records_host(files)
    d.set_tables(tabs, form["sampling"], form["Ri"])
    B, H, W = len(files), form["H"], form["W"]
    dev = [torch.from_numpy(a).cuda() for a in (blob, offsets, recs)]
    out = torch.full((B, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    d.decode_dev(*dev, B, H, W, out, out.numel(), status)
    d.sync()
    return out.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("sub", [4, None], ids=["sub4", "default"])
def test_eight_frames_of_several_windows_streamed_and_resident(sub):
    files = [DC.pillow_jpeg(64, 64, "444", 95, 0, False, s) for s in range(8)]
    assert all(MJ.parse(j)["Ri"] == 0 and len(j) > 9000 for j in files)       # about 10 KB: ten windows of 256 lanes at sub 4
    want = np.stack([DC.twin(j)[0] for j in files])
    for j in files[:2]:
        out, st, stats = SC.split(j, sub or 0, 256, stats=True)
        assert st == 0 and np.array_equal(out, DC.twin(j)[0]) and (stats["windows"] >= 9 if sub == 4 else stats["windows"] >= 1)
    d = MJ.MjpegDecoder(chunk=3, split="auto", sub=sub)
    got, st = d.decode(files, statuses=True)
    assert not st.any() and np.array_equal(got, want)
    res, st = d.decode_resident(files, statuses=True)
    assert res.is_cuda and not st.any() and np.array_equal(res.cpu().numpy(), want)
    frames, st = _resident(d, files)
    assert not st.any() and np.array_equal(frames, want)
    d.set_split("off")                                                        # the same handle, the lane per interval
    got, st = d.decode(files, statuses=True)
    assert not st.any() and np.array_equal(got, want)


@pytest.mark.parametrize("form", list(DC.FORMS))
@pytest.mark.parametrize("H,W", [(37, 50), (17, 9)])
def test_the_four_forms(H, W, form):
    files = [DC.pillow_jpeg(H, W, form, q, 0, opt) for q, opt in ((75, False), (100, True), (30, False))]
    want = np.stack([DC.twin(j)[0] for j in files])
    for sub in (4, 8, None):
        got, st = MJ.MjpegDecoder(split="auto", sub=sub).decode(files, statuses=True)
        assert not st.any() and np.array_equal(got, want), sub


def test_damaged_frames_beside_an_intact_one_under_guard_zones():
    """37x50 gray: intact, truncated mid-scan, an invalid code, a DC prediction out of range.  The twin's statuses and pixels, the
    neighbours untouched, inputs and outputs inside guard zones."""
    hand = SC.handmade(37, 50)
    intact = hand["intact"][0]
    lo, hi = DC.scan_span(intact)
    files = [intact, intact[:(lo + hi) // 2], hand["invalid-then-dc-overflow"][0], hand["dc-overflow"][0], hand["zrl-overflow"][0], intact]
    want = [DC.twin(j) for j in files]
    assert [st for _, st in want] == [0, 1, 2, 4, 3, 0]
    for sub in (4, 64):
        for j, (f, s) in zip(files, want):
            out, st = SC.split(j, sub, 256)
            assert st == s and np.array_equal(out, f)
        d = MJ.MjpegDecoder(split="auto", sub=sub)
        blob, offsets, recs, tabs, form = MJ.records_host(files)
        assert (form["H"], form["W"], form["Ri"]) == (37, 50, 0)
        d.set_tables(tabs, form["sampling"], form["Ri"])
        B, H, W = len(files), 37, 50
        out = G.run_guarded("og_mjpd_decode_u8_dev", f"split sub {sub}",
                            lambda p: lib().og_mjpd_decode_u8_dev(d._h, p["blob"], p["offsets"], p["recs"], B, H, W, p["frames"], B * H * W * 3, p["status"]),
                            {"blob": blob, "offsets": offsets, "recs": recs}, {"frames": B * H * W * 3, "status": 4 * B}, kind="device", sync=d.sync)
        assert out["status"].view(np.int32).tolist() == [0, 1, 2, 4, 3, 0]
        frames = out["frames"].reshape(B, H, W, 3)
        for i, (f, _) in enumerate(want):
            assert np.array_equal(frames[i], f), (sub, i)
        got, st = d.decode(files, statuses=True)                              # the streamed entry
        assert st.tolist() == [0, 1, 2, 4, 3, 0] and all(np.array_equal(got[i], want[i][0]) for i in range(B))


# ── the kernel's windows: staging, the data-end search and the lane masks exist only on the device ─────────────────────────────────
# Every case: device = the sequential twin = the split twin at the kernel's lanes per window, statuses and bytes.  The files and
# their firing checks (the case holds what it is named for) are tests/mjps_cases.py's, held to the twins on the CPU by
# tests/test_mjps_host.py.
def _judge(files, sub, frames, status, what):
    assert len(frames) == len(status) == len(files)
    for i, j in enumerate(files):
        ref, st = DC.twin(j)
        out, st2, _ = SC.kernel_twin(j, sub)
        assert int(status[i]) == st == st2, (what, sub, i, int(status[i]), st, st2)
        assert np.array_equal(frames[i], ref) and np.array_equal(frames[i], out), (what, sub, i)


def _guarded(d, blob, offsets, recs, B, H, W, label):
    """The raw entry inside guard zones (buffer_guard.run_guarded: three runs, the slack 0x00 and 0xFF): `(frames, status)`."""
    out = G.run_guarded("og_mjpd_decode_u8_dev", label,
                        lambda p: lib().og_mjpd_decode_u8_dev(d._h, p["blob"], p["offsets"], p["recs"], B, H, W, p["frames"], B * H * W * 3, p["status"]),
                        {"blob": blob, "offsets": offsets, "recs": recs}, {"frames": B * H * W * 3, "status": 4 * B}, kind="device", sync=d.sync)
    return out["frames"].reshape(B, H, W, 3), out["status"].view(np.int32)


def _three_entries(d, files, sub, what):
    """The streamed entry, decode_resident and the raw og_mjpd_decode_u8_dev call."""
    got, st = d.decode(files, statuses=True)
    _judge(files, sub, got, st, what + ": streamed")
    res, st = d.decode_resident(files, statuses=True)
    assert res.is_cuda
    _judge(files, sub, res.cpu().numpy(), st, what + ": decode_resident")
    frames, st = _resident(d, files)
    _judge(files, sub, frames, st, what + ": decode_dev")


@pytest.mark.parametrize("name,sub", [(n, s) for n, v in SC.REAL.items() for s in v[3]], ids=lambda v: str(v))
def test_real_windows_at_every_sub(name, sub):
    """Pillow noise at quality 100 without DRI: 67 KB (128 x 128, three windows at the large subs) and 101 KB (128 x 192) in 4:4:4,
    and the larger shape in 4:2:0 and gray, whose base and predictors carry over MCUs of six blocks and of one.  At sub 256, 512
    and 1024 a full window has 128, 64 and 32 lanes: the rest of the workgroup is idle."""
    j = SC.real_fires(name)
    d = MJ.MjpegDecoder(split="auto", sub=sub)
    _three_entries(d, [j], sub, name)
    d.set_split("off")                                                        # the same handle, the lane per interval
    got, st = d.decode([j], statuses=True)
    assert not st.any() and np.array_equal(got[0], DC.twin(j)[0])


@pytest.mark.parametrize("sub", [256, 4])
def test_frames_of_different_window_counts_in_one_launch(sub):
    """chunk 3, five frames: each workgroup leaves its window loop on its own -- after three windows, after one short one, at an
    error in its second."""
    files = list(SC.mixed_fires(sub))
    d = MJ.MjpegDecoder(chunk=3, split="auto", sub=sub)
    got, st = d.decode(files, statuses=True)
    _judge(files, sub, got, st, "mixed: streamed")
    res, st = d.decode_resident(files, statuses=True)
    _judge(files, sub, res.cpu().numpy(), st, "mixed: decode_resident")
    assert st.tolist() == [0, 0, 0, 0, 1]


@pytest.mark.parametrize("sub", [4, 8])
def test_bytes_placed_at_window_edges(sub):
    """Hand-made gray scans, windows of 1024 and 2048 bytes: a stuffed pair across Wn and across 2 Wn, one whose FF is the last
    staged byte of window 0, one on a dword edge of the end search, a lane of window 1 that starts on the 00; the data end at Wn - 1,
    Wn, Wn + 1, Wn + K - 1, Wn + K and Wn + K + 1 in a complete frame (the FF has to be found; behind Wn a second window of one to
    five lanes), the same six lengths as truncated scans that end without any FF, and a truncated scan of exactly Wn bytes whose last
    symbol ends with its last bit: there only the open end of window 0's last lane finds the missing bits."""
    d = MJ.MjpegDecoder(split="auto", sub=sub)
    _three_entries(d, [SC.edge_fires(n, sub) for n in SC.EDGES], sub, "edges")
    for part in (SC.ENDS[:3], SC.ENDS[3:]):
        _three_entries(d, [SC.end_fires(n, sub) for n in part], sub, f"ends {part}")
        _three_entries(d, [SC.cut_fires(n, sub) for n in part], sub, f"cuts {part}")
    _three_entries(d, [SC.symbol_edge_fires(sub)], sub, "a scan of exactly Wn bytes that ends on a symbol's last bit")


def test_a_hand_made_scan_of_three_windows_at_sub_1024():
    """384 blocks of 63 ten-bit AC values, 77 KB: every lane of 1024 bytes holds five blocks."""
    j = SC.three_windows_at_1024()
    assert SC.kernel_twin(j, 1024)[2]["windows"] >= 3
    for sub in (1024, 512):
        _three_entries(MJ.MjpegDecoder(split="auto", sub=sub), [j], sub, "three windows at 1024")


@pytest.mark.parametrize("built_for", [4, 8])
def test_errors_behind_window_0_under_guard_zones(built_for):
    """64 x 128 gray: a truncation, a ZRL past 63 and a DC prediction out of range in window 1, an invalid code in window 2, an
    intact neighbour on each side; base, pred0 and the carry are not 0 where the error key is made and the erase pass runs.  The files
    built for the windows of one sub also run at the other."""
    for name in SC.late_errors(built_for):
        SC.late_fires(name, built_for)
    for sub in (4, 8):
        d = MJ.MjpegDecoder(split="auto", sub=sub)
        for names in SC.LATE_BATCHES:
            cases = [SC.late_errors(built_for)[n] for n in names]
            files = [j for j, _, _ in cases]
            blob, offsets, recs, tabs, form = MJ.records_host(files)
            assert (form["H"], form["W"], form["Ri"]) == (64, 128, 0)
            d.set_tables(tabs, form["sampling"], form["Ri"])
            frames, st = _guarded(d, blob, offsets, recs, len(files), 64, 128, f"late errors of sub {built_for} at sub {sub}")
            assert st.tolist() == [claim for _, claim, _ in cases]
            _judge(files, sub, frames, st, f"late {names}")
            got, st = d.decode(files, statuses=True)
            _judge(files, sub, got, st, f"late {names}: streamed")


@pytest.mark.parametrize("which", ["hand-made, sub 4", "pillow, sub 256"])
def test_the_four_source_alignments(which):
    """The caller owns `offsets`: the same file at four consecutive bytes of the blob, so that the staging's `a` (the scan's address
    modulo 4) takes every value; the bytes around the file are 0x00 in one guarded run and 0xFF in the other."""
    sub = 4 if which.startswith("hand") else 256
    j = SC.edge_fires("pair-across-Wn", 4) if sub == 4 else SC.real_fires("444-128x128")
    assert SC.kernel_twin(j, sub)[2]["windows"] >= 3
    info = MJ.parse(j)
    H, W = info["H"], info["W"]
    _, offsets, recs, tabs, form = MJ.records_host([j])
    d = MJ.MjpegDecoder(split="auto", sub=sub)
    d.set_tables(tabs, form["sampling"], form["Ri"])
    seen = set()
    for o in range(64, 68):
        shifted = offsets + o
        seen.add(int(shifted[0] + recs[0, 0]) & 3)
        blob = lambda fill, o=o: np.concatenate([np.full(o, fill, np.uint8), np.frombuffer(j, np.uint8), np.full(61, fill, np.uint8)])
        frames, st = _guarded(d, blob, shifted, recs, 1, H, W, f"{which}, file at byte {o}")
        _judge([j], sub, frames, st, f"file at byte {o}")
    assert recs[0, 0] == info["scan_offset"] and seen == {0, 1, 2, 3}


def test_files_with_restart_markers_take_the_old_kernel():
    files = [DC.pillow_jpeg(37, 50, "420", 75, 1, False, s) for s in range(3)]
    want = np.stack([DC.twin(j)[0] for j in files])
    on, off = MJ.MjpegDecoder(split="auto", sub=4), MJ.MjpegDecoder()
    a, sa = on.decode(files, statuses=True)
    b, sb = off.decode(files, statuses=True)
    assert np.array_equal(a, b) and np.array_equal(a, want) and sa.tolist() == sb.tolist() == [0, 0, 0]
    assert on.plan(3, 37, 50, 3, 1) == off.plan(3, 37, 50, 3, 1)
    damaged = list(DC.status_cases())                                         # Ri = 1: truncated, invalid code, a missing RSTm
    a, sa = on.decode(damaged, statuses=True)
    b, sb = off.decode(damaged, statuses=True)
    assert np.array_equal(a, b) and sa.tolist() == sb.tolist() == [0, 1, 2, 5]


def test_cli_infer_with_decode_split_writes_what_the_host_path_writes(tmp_path, monkeypatch):
    """`--pipeline unet-only --decode device --decode-split auto` on a Pillow-written 64 x 64 .avi without DRI."""
    import os
    import sys

    from openglottal_amd import cli, synth

    monkeypatch.setitem(sys.modules, "cv2", None)
    feats = (32, 64, 128, 256)
    torch.save(synth.state_dict_to_torch(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5)), tmp_path / "unet.pt")
    files = [DC.pillow_jpeg(64, 64, "420", 75, 0, False, s) for s in range(6)]
    assert all(MJ.parse(j)["Ri"] == 0 for j in files)
    os.makedirs(tmp_path / "in")
    with MJ.AviWriter(str(tmp_path / "in" / "clip.avi"), 64, 64) as w:
        w.write(np.frombuffer(b"".join(files), np.uint8), [len(j) for j in files])
    base = ["infer", "--input", str(tmp_path / "in"), "--pipeline", "unet-only", "--unet-weights", str(tmp_path / "unet.pt")]
    seen = []
    real = MJ.MjpegDecoder.set_split
    monkeypatch.setattr(MJ.MjpegDecoder, "set_split", lambda self, split="off", sub=None: seen.append(split) or real(self, split, sub))
    assert cli.main(base + ["--output-dir", str(tmp_path / "host"), "--decode", "host"]) == 0
    assert cli.main(base + ["--output-dir", str(tmp_path / "split"), "--decode", "device", "--decode-split", "auto"]) == 0
    assert seen == ["auto"]
    assert sorted(os.listdir(tmp_path / "split")) == sorted(os.listdir(tmp_path / "host")) == ["clip_out.npy", "features.csv"]
    assert open(tmp_path / "split" / "features.csv").read() == open(tmp_path / "host" / "features.csv").read()
    assert np.array_equal(np.load(tmp_path / "split" / "clip_out.npy"), np.load(tmp_path / "host" / "clip_out.npy"))
