"""-m gpu: baseline JPEG decoded on the device (include/decode/openglottal_hip_mjpd.h).  Device bytes = the host twin's bytes in every
case, in the smallest shapes where each mechanism can still go wrong; tests/test_mjpd_host.py holds the twin to Pillow."""
import numpy as np
import pytest
import torch

import buffer_guard as G
import mjpd_cases as DC
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import OpenGlottalHipError, check, lib

pytestmark = pytest.mark.gpu

# (H, W, form, MCUs per restart interval): edge replication, odd chroma extents and a single MCU; a ragged last interval; one lane per
# frame; 256 intervals, more than one wave of lanes per frame
SHAPES = [(H, W, form, 0) for H, W in ((8, 8), (17, 9)) for form in ("gray", "444", "422", "420")] + \
         [(37, 50, "420", 1), (37, 50, "420", 3), (64, 64, "420", 0), (128, 128, "444", 1)]


@pytest.fixture(scope="module")
def decoder():
    return MJ.MjpegDecoder()


@pytest.mark.parametrize("H,W,form,restart", SHAPES, ids=lambda v: str(v))
def test_device_bytes_are_the_twins(decoder, H, W, form, restart):
    j = DC.pillow_jpeg(H, W, form, 75, restart)
    info = MJ.parse(j)
    assert (info["sampling"], info["Ri"]) == (DC.SAMPLING[form], restart)
    if (H, W, restart) == (128, 128, 1):
        assert info["nI"] == 256
    want, st = DC.twin(j)
    assert st == 0
    got = decoder.decode([j])
    assert got.shape == (1, H, W, 3) and np.array_equal(got[0], want)
    res = decoder.decode_resident([j, j])
    assert res.is_cuda and np.array_equal(res.cpu().numpy(), np.stack([want, want]))


def test_per_frame_tables_and_a_ragged_last_micro_batch():
    files = [DC.pillow_jpeg(37, 50, "420", q, 0, opt, seed) for seed, (q, opt) in enumerate(((30, False), (95, True), (75, True), (1, False), (100, True)))]
    assert len({len(j) for j in files}) == 5
    _, _, recs, tabs, form = MJ.records_host(files)
    assert tabs.shape[0] == 5 and recs[:, 3].tolist() == [0, 1, 2, 3, 4] and form["sampling"] == 3
    d = MJ.MjpegDecoder(chunk=2)
    want = np.stack([DC.twin(j)[0] for j in files])
    assert np.array_equal(d.decode(files), want)
    assert np.array_equal(d.decode_resident(files).cpu().numpy(), want)
    # one table set shared by every frame, and a set that the first lane of a workgroup does not use
    again = [files[0], files[0], files[1], files[0], files[0]]
    assert MJ.records_host(again)[3].shape[0] == 2
    assert np.array_equal(d.decode(again), want[[0, 0, 1, 0, 0]])


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def test_round_trip_through_the_device_encoder(decoder):
    src = np.stack([DC.noise(40, 56, s) for s in range(3)])
    blob, sizes = MJ.Mjpeg(quality=75).encode_resident(torch.from_numpy(src.copy()).cuda())
    files = MJ.split(blob, sizes)
    assert MJ.parse(files[0])["Ri"] == 16 and MJ.parse(files[0])["sampling"] == 1
    got = decoder.decode_resident(files).cpu().numpy()
    for i, j in enumerate(files):
        assert np.array_equal(got[i], DC.twin(j)[0])
        assert abs(psnr(got[i], src[i]) - psnr(DC.pillow_bgr(j), src[i])) <= 0.1


def _resident_call(d, files, H, W, label):
    blob, offsets, recs, tabs, form = MJ.records_host(files)
    assert (form["H"], form["W"]) == (H, W)
    d.set_tables(tabs, form["sampling"], form["Ri"])
    B = len(files)
    out = G.run_guarded("og_mjpd_decode_u8_dev", label,
                        lambda p: lib().og_mjpd_decode_u8_dev(d._h, p["blob"], p["offsets"], p["recs"], B, H, W, p["frames"], B * H * W * 3, p["status"]),
                        {"blob": blob, "offsets": offsets, "recs": recs}, {"frames": B * H * W * 3, "status": 4 * B}, kind="device", sync=d.sync)
    return out["frames"].reshape(B, H, W, 3), out["status"].view(np.int32)


def test_statuses_and_pixels_of_damaged_frames_are_the_twins(decoder):
    """Frame 0 intact, 1 truncated mid-scan, 2 with an invalid code, 3 without its RSTm: cases the twin has passed (the same inline
    function), under guard zones on the frames and the statuses, the blob padded with slack of 0x00 and then 0xFF."""
    files = list(DC.status_cases())
    want = [DC.twin(j) for j in files]
    assert [st for _, st in want] == [0, 1, 2, 5]
    frames, status = _resident_call(decoder, files, 17, 9, "statuses")
    assert status.tolist() == [0, 1, 2, 5]
    for i, (f, _) in enumerate(want):
        assert np.array_equal(frames[i], f), i
    assert np.array_equal(frames[0], DC.pillow_bgr(files[0]))
    # the streamed entry: the same, and the Python layer names the first damaged frame
    got, st = decoder.decode(files, statuses=True)
    assert st.tolist() == [0, 1, 2, 5] and all(np.array_equal(got[i], want[i][0]) for i in range(4))
    with pytest.raises(OpenGlottalHipError, match="frame 1 of 4.*truncated scan"):
        decoder.decode(files)


def test_refused_and_foreign_frames_do_not_stop_their_neighbours(decoder):
    good = DC.pillow_jpeg(17, 9, "420", 75, 1)
    import io

    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(DC.noise(17, 9)).save(b, "JPEG", progressive=True)
    files = [good, b.getvalue(), DC.pillow_jpeg(8, 8, "420", 75, 1), good]
    got, st = decoder.decode(files, statuses=True)
    assert st.tolist() == [0, 6, 7, 0]
    assert np.array_equal(got[0], DC.twin(good)[0]) and np.array_equal(got[3], got[0]) and not got[1].any() and not got[2].any()
    with pytest.raises(OpenGlottalHipError, match="frame 1 of 4.*progressive"):
        decoder.decode(files)


def test_cli_infer_decodes_on_the_device_and_writes_what_the_host_path_writes(tmp_path, capsys, monkeypatch):
    """`--pipeline unet-only --decode device` on a 6-frame 64 x 64 .avi written by `AviWriter`: the same features.csv and _out.npy as
    `--decode host`, whose frames are Pillow's; the decoded block is the pipeline's `src` and never visits the host."""
    import os
    import sys

    from openglottal_amd import cli, synth
    from openglottal_amd import infer as I

    monkeypatch.setitem(sys.modules, "cv2", None)                         # no OpenCV, wherever this runs: the host path is the RIFF walk + Pillow
    feats = (32, 64, 128, 256)
    torch.save(synth.state_dict_to_torch(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5)), tmp_path / "unet.pt")
    files = [MJ.encode_host(DC.noise(64, 64, s) // 2 + 40, 75) for s in range(6)]
    os.makedirs(tmp_path / "in")
    with MJ.AviWriter(str(tmp_path / "in" / "clip.avi"), 64, 64) as w:
        w.write(np.frombuffer(b"".join(files), np.uint8), [len(j) for j in files])
    base = ["infer", "--input", str(tmp_path / "in"), "--pipeline", "unet-only", "--unet-weights", str(tmp_path / "unet.pt")]
    uploads = []
    real = I._block_array
    monkeypatch.setattr(I, "_block_array", lambda blk: uploads.append(len(blk)) or real(blk))
    assert cli.main(base + ["--output-dir", str(tmp_path / "host"), "--decode", "host"]) == 0
    assert uploads == [6]                                                 # the host path uploads the decoded block
    assert cli.main(base + ["--output-dir", str(tmp_path / "dev"), "--decode", "device"]) == 0
    assert uploads == [6]                                                 # the device path uploads no decoded frame
    assert cli.main(base + ["--output-dir", str(tmp_path / "auto"), "--decode", "auto"]) == 0
    assert uploads == [6] and "--decode auto" not in capsys.readouterr().err
    for d in ("dev", "auto"):
        assert sorted(os.listdir(tmp_path / d)) == sorted(os.listdir(tmp_path / "host")) == ["clip_out.npy", "features.csv"]
        assert open(tmp_path / d / "features.csv").read() == open(tmp_path / "host" / "features.csv").read()
        assert np.array_equal(np.load(tmp_path / d / "clip_out.npy"), np.load(tmp_path / "host" / "clip_out.npy"))
    assert np.load(tmp_path / "host" / "clip_out.npy").shape == (6, 64, 64, 3)


def test_iter_avi_blocks_and_the_resident_python_entry(tmp_path, decoder):
    """`mjpeg.iter_avi_blocks`: the RIFF walk handing 4 files at a time to the decoder, a ragged last block, on the host and resident;
    a directory of .jpg files the same; and `MjpegDecoder.decode_dev` after `set_tables`."""
    import os

    files = [MJ.encode_host(DC.noise(24, 40, s), 75) for s in range(10)]
    want = np.stack([DC.twin(j)[0] for j in files])
    with MJ.AviWriter(str(tmp_path / "clip.avi"), 40, 24) as w:
        w.write(np.frombuffer(b"".join(files), np.uint8), [len(j) for j in files])
    os.makedirs(tmp_path / "seq")
    for i, j in enumerate(files):
        (tmp_path / "seq" / f"{i:03d}.jpg").write_bytes(j)
    for path in (tmp_path / "clip.avi", tmp_path / "seq"):
        got = list(MJ.iter_avi_blocks(str(path), 4, decoder))
        assert [b0 for b0, _ in got] == [0, 4, 8] and [len(f) for _, f in got] == [4, 4, 2]
        assert all(isinstance(f, np.ndarray) for _, f in got) and np.array_equal(np.concatenate([f for _, f in got]), want)
    res = list(MJ.iter_avi_blocks(str(tmp_path / "clip.avi"), 4, decoder, resident=True))
    assert all(f.is_cuda for _, f in res) and np.array_equal(torch.cat([f for _, f in res]).cpu().numpy(), want)
    video = MJ.open_compressed(str(tmp_path / "clip.avi"))
    assert (len(video), video.H, video.W) == (10, 24, 40) and np.array_equal(video.frames_host(3), want) and np.array_equal(video[7], want[7])

    blob, offsets, recs, tabs, form = MJ.records_host(files)
    decoder.set_tables(tabs, form["sampling"], form["Ri"])
    dev = [torch.from_numpy(a).cuda() for a in (blob, offsets, recs)]
    out = torch.full((10, 24, 40, 3), 7, dtype=torch.uint8, device="cuda")
    status = torch.full((10,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    decoder.decode_dev(*dev, 10, 24, 40, out, out.numel(), status)
    decoder.sync()
    assert not status.any() and np.array_equal(out.cpu().numpy(), want)
