"""-m gpu: k_mjps_entropy (include/split/openglottal_hip_mjps.h), the split entropy pass of files without restart markers.  Device bytes
and statuses = the split twin's = the sequential twin's = the same handle's with the mode off, in the smallest shapes where each
mechanism can go wrong: several windows at sub 4, every form, damaged frames beside an intact one under guard zones."""
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
