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
    j2 = DC.pillow_jpeg(H, W, form, 75, restart, False, 1)       # a second seed: two frames exchanged, or one decoded twice, would show
    want2, st2 = DC.twin(j2)
    assert st2 == 0 and not np.array_equal(want2, want)
    res = decoder.decode_resident([j, j2])
    assert res.is_cuda and np.array_equal(res.cpu().numpy(), np.stack([want, want2]))


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


# ── what the twin does not share with the device: k_mjpd_markers' strides and ballots, k_mjpd_entropy's lane map ───────────────────────
# The files and the predicates that make each of them the case it is named for are tests/mjpd_cases.py's (asserted by every builder,
# and again in tests/test_mjpd_host.py, where the valid ones are held to Pillow).
def _wanted(files):
    """The twins' `(frames, statuses)`; a frame the twin refuses is all zero."""
    H, W = next(f.shape[:2] for f, _ in map(DC.twin, files) if f is not None)
    frames = np.stack([DC.twin(j)[0] if DC.twin(j)[0] is not None else np.zeros((H, W, 3), np.uint8) for j in files])
    return frames, [DC.twin(j)[1] for j in files]


def _first_difference(got, want, labels=None):
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    return [(i, labels[i] if labels else None) for i in bad[:8]]


def _dev_call(d, files, H, W):
    """`decode_dev` after `set_tables`: frames and statuses, pre-filled with values no decode leaves."""
    blob, offsets, recs, tabs, form = MJ.records_host(files)
    d.set_tables(tabs, form["sampling"], form["Ri"])
    dev = [torch.from_numpy(a).cuda() for a in (blob, offsets, recs)]
    B = len(files)
    out = torch.full((B, H, W, 3), 7, dtype=torch.uint8, device="cuda")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    d.decode_dev(*dev, B, H, W, out, out.numel(), status)
    d.sync()
    return out.cpu().numpy(), status.cpu().numpy()


def _every_entry(files, H, W, chunk=128, labels=None):
    """Device = twins, statuses and bytes, through `decode`, `decode_resident` and `decode_dev`."""
    want, sts = _wanted(files)
    d = MJ.MjpegDecoder(chunk=chunk)
    got, st = d.decode(files, statuses=True)
    assert st.tolist() == sts and not _first_difference(got, want, labels), ("decode", chunk, st.tolist(), _first_difference(got, want, labels))
    got, st = d.decode_resident(files, statuses=True)
    assert st.tolist() == sts and not _first_difference(got.cpu().numpy(), want, labels), ("decode_resident", chunk, st.tolist())
    got, st = _dev_call(d, files, H, W)
    assert st.tolist() == sts and not _first_difference(got, want, labels), ("decode_dev", chunk, st.tolist())
    return want, sts


def test_markers_many_to_a_wave_and_the_write_guard(decoder):
    """[dense, doubled-all, dense', renumbered-late, dense, doubled-all], 8 x 2400 gray with nI = 300: up to 19 markers in one wave's
    ballot, markers in all four waves of a stride, 299 of them (k & 7 wraps 37 times).  doubled-all has 598: without `k + 1 < nI`
    its surplus would be written into the next frame's interval table and, from the last frame, into mstat[0..]."""
    files = DC.guard_batch()
    want, sts = _wanted(files)
    assert sts == DC.GUARD_STATUS == [0, 5, 0, 5, 0, 5] and not np.array_equal(want[2], want[0])
    frames, status = _resident_call(decoder, files, 8, 2400, "markers-guard")
    assert status.tolist() == sts
    assert not _first_difference(frames, want, DC.GUARD_ORDER), _first_difference(frames, want, DC.GUARD_ORDER)
    assert np.array_equal(frames[0], frames[4]) and not np.array_equal(frames[2], frames[0]) and (frames[[1, 3, 5]] == 128).all()
    for chunk in (2, 128):
        got, st = MJ.MjpegDecoder(chunk=chunk).decode(files, statuses=True)
        assert st.tolist() == sts and not _first_difference(got, want, DC.GUARD_ORDER), (chunk, st.tolist())


def test_markers_damaged_behind_the_first_stride(decoder):
    """Every damage of dense(0) between intact neighbours: a wrong number at marker 200, one wrong by 4 at marker 201 (right in its
    low two bits), k % 7 from marker 8 on, the last marker
    missing, FF D3 as the scan's last two bytes (i = n - 2), and a scan that ends in a lone FF (i = n - 1, status 0): behind it lies
    a two-byte 'file' D0 D0 that the parser refuses, so a lane that read p[n] would find a marker there."""
    cases = DC.damaged()
    names = ["renumbered-late", "renumbered-by-4", "mod7", "removed-last", "end-marker", "ff-last"]
    files, labels = [DC.dense(1)], ["dense'"]
    for n in names:
        files += [cases[n][0]] + ([b"\xd0\xd0"] if n == "ff-last" else []) + [DC.dense(0)]
        labels += [n] + (["D0 D0"] if n == "ff-last" else []) + ["dense"]
    want, sts = _wanted(files)
    assert sts == [0, 5, 0, 5, 0, 5, 0, 5, 0, 5, 0, 0, 6, 0]
    frames, status = _resident_call(decoder, files, 8, 2400, "markers-damaged")
    assert status.tolist() == sts and not _first_difference(frames, want, labels), (status.tolist(), _first_difference(frames, want, labels))
    got, st = decoder.decode(files, statuses=True)
    assert st.tolist() == sts and not _first_difference(got, want, labels)


def test_markers_on_stride_and_wave_edges_and_scan_lengths(decoder):
    """8 x 96 gray, Ri = 1: a marker whose FF is byte 255, 254, 0, 63 or 64 of a stride (two seeds each), and scans of 0, 1 and 255
    bytes mod 256 (the tail test i + 1 < n), in one call; every file is valid."""
    files = [(f"edge-{R}-{w}", DC.edge_case(R, w)) for R in DC.EDGES for w in (0, 1)] + [(f"length-{r}", DC.length_case(r)) for r in DC.LENGTHS]
    labels, files = [n for n, _ in files], [j for _, j in files]
    want, sts = _wanted(files)
    assert sts == [0] * 13 and len({f.tobytes() for f in want}) == 13
    frames, status = _resident_call(decoder, files, 8, 96, "markers-edges")
    assert status.tolist() == sts and not _first_difference(frames, want, labels), (status.tolist(), _first_difference(frames, want, labels))
    got, st = MJ.MjpegDecoder(chunk=3).decode(files, statuses=True)
    assert st.tolist() == sts and not _first_difference(got, want, labels)


def test_markers_behind_strides_without_any(decoder):
    """Intervals longer than a stride: `base` is carried over whole strides and wave slices that hold no marker."""
    files = [DC.sparse(0), DC.sparse(1)]
    H, W, _ = DC.SPARSE_SHAPE
    assert all(DC.empty_strides(j) and DC.empty_slices(j) for j in files)
    want, sts = _wanted(files)
    assert sts == [0, 0] and not np.array_equal(want[0], want[1])
    frames, status = _resident_call(decoder, files, H, W, "markers-sparse")
    assert status.tolist() == sts and not _first_difference(frames, want)
    assert np.array_equal(decoder.decode(files), want)


def test_lane_map_a_workgroup_that_starts_inside_a_frame():
    """Seven distinct 37 x 50 4:2:0 frames of seven table sets, nI = 12: 84 lanes, the second workgroup starts at frame 5, interval 4,
    with frame 5's set in LDS and frame 6's read from global memory."""
    files = list(DC.lane_files())
    assert MJ.records_host(files)[3].shape[0] == 7 and 64 // MJ.parse(files[0])["nI"] == 5
    _, sts = _every_entry(files, 37, 50)
    assert sts == [0] * 7
    # frame 5 damaged: the second workgroup's first frame is refused by k_mjpd_markers (set0 = -1), frame 6 decodes from global tables
    broken = files[:5] + [DC.rst_removed(files[5])] + files[6:]
    _, sts = _every_entry(broken, 37, 50)
    assert sts == [0, 0, 0, 0, 0, 5, 0]
    # frames 5 and 6 are frame 0's file: the second workgroup's LDS set is one that the first workgroup used too
    shared = files[:5] + [files[0], files[0]]
    assert MJ.records_host(shared)[3].shape[0] == 5 and MJ.records_host(shared)[2][:, 3].tolist() == [0, 1, 2, 3, 4, 0, 0]
    _every_entry(shared, 37, 50)
    # 36 lanes per micro-batch: three micro-batches through both slots
    _every_entry(files, 37, 50, chunk=3)


@pytest.mark.parametrize("nI", (3, 20))
def test_lane_map_at_an_interval_count_that_does_not_divide_64(nI):
    files, lane64 = DC.lane_batch(nI)
    assert MJ.parse(files[0])["nI"] == nI and 64 % nI and lane64 == (64 // nI, 64 % nI) and lane64[0] < len(files)
    _, sts = _every_entry(files, 37, 50)
    assert sts == [0] * len(files)


def _corpus_call(decoder, name):
    base = DC.bases()[0 if name == "ri1" else 1]
    files = [(f"{name}-base", base)] + [(label, j) for label, j in DC.hostile() if label.startswith(name + "-")]
    labels, files = [n for n, _ in files], [j for _, j in files]
    want, sts = _wanted(files)
    got, st = decoder.decode(files, statuses=True)
    wrong = [(labels[i], int(st[i]), sts[i]) for i in np.flatnonzero(st != np.asarray(sts))]
    assert not wrong, wrong[:8]
    assert not _first_difference(got, want, labels), _first_difference(got, want, labels)
    assert not got[np.asarray(sts) == 6].any()
    return sts


def test_the_whole_hostile_corpus_ri1(decoder):
    """The intact Ri = 1 base and all of its 1 285 damaged copies in one streamed call: every status and every frame the twin's."""
    sts = _corpus_call(decoder, "ri1")
    assert len(sts) == 1 + len(DC.bases()[0]) + 500 + 3 == 1286 and set(sts) >= {0, 1, 2, 3, 5, 6}


def test_the_whole_hostile_corpus_nodri(decoder):
    sts = _corpus_call(decoder, "nodri")
    assert len(sts) == 1 + len(DC.bases()[1]) + 500 == 1275 and set(sts) >= {0, 1, 2, 3, 6}


def test_narrow_planes_and_one_pixel_frames(decoder):
    """Chroma of one or two columns (og_jpegd_chroma's replication branch) and of three (the first filtered one); 1 x 1 frames, where a
    k_mjpd_idct workgroup has 8 to 24 live lanes per frame.  Three distinct seeds per call."""
    assert {(W + 1) // 2 for _, W, form in DC.NARROW if form in ("422", "420")} == {1, 2, 3}
    for H, W, form in DC.NARROW:
        files = DC.narrow_files(H, W, form)
        want, sts = _wanted(files)
        assert sts == [0, 0, 0], (H, W, form)
        got = decoder.decode_resident(files)
        assert got.shape == (3, H, W, 3) and np.array_equal(got.cpu().numpy(), want), (H, W, form)
        assert np.array_equal(decoder.decode(files), want), (H, W, form)


def test_long_codes_from_lds_and_from_global_memory(decoder):
    """Codes of 10..16 bits miss the 9-bit look-up; og_jpegd_symbol then walks maxcode/valoff/vals -- in the LDS copy when the frame's
    set is the workgroup's first, in global memory otherwise.  The past-the-bound file has another table set (its DQT)."""
    j, lengths = DC.long_codes()
    assert lengths == tuple(DC.long_lengths(DC._dht(j)[(1, 0)])) and max(lengths) == 16 and sum(n >= 10 for n in lengths) >= 3
    other = DC.past_the_bound()
    for files in ([j, other, j], [other, j]):
        assert MJ.records_host(files)[3].shape[0] == 2
        want, sts = _wanted(files)
        assert sts == [0] * len(files)
        assert np.array_equal(decoder.decode(files), want)
    c = DC.long_chroma()
    assert max(DC.long_lengths(DC._dht(c)[(1, 1)])) > 9
    files = [c, DC.pillow_jpeg(37, 50, "444", 95, 0, True, 4), c]
    want, sts = _wanted(files)
    assert sts == [0, 0, 0] and np.array_equal(decoder.decode_resident(files).cpu().numpy(), want)


def test_past_the_bound_the_device_wraps_as_the_twin_does(decoder):
    """Outside the header's BOUND only device = twin is claimed: uint32 wrap-around in both passes of og_jpegd_idct8."""
    j = DC.past_the_bound()
    want, sts = _wanted([j, j])
    assert sts == [0, 0] and len(np.unique(want[0])) > 1
    frames, status = _resident_call(decoder, [j, j], 8, 64, "past-the-bound")
    assert status.tolist() == [0, 0] and np.array_equal(frames, want)
    files = [DC._handmade_gray(dc, 255) for dc in (1023, -1023, 2047, -2047)]
    want, sts = _wanted(files)
    assert sts == [0] * 4
    assert np.array_equal(decoder.decode(files), want)
