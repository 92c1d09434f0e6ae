"""-m gpu: `infer.iter_pipeline_mjpeg` and `cli infer --avi device` against what the project already has: the JPEG files equal the host
twin's encoding of `run_pipeline`'s annotated frames byte for byte, the areas are identical, the AVI passes the RIFF walk and holds
those bytes, and without the flag the output directory holds what it held before.  Seeded nets as tests/test_gpu_infer.py builds
them; 12 frames in two blocks at 256 x 256 and at 96 x 80."""
import csv
import os
import struct
import sys

import numpy as np
import pytest
import torch

import crop_cases as K
import mjpeg_cases as MC
import openglottal_amd as og
from openglottal_amd import cli
from openglottal_amd import features as F
from openglottal_amd import infer as I
from openglottal_amd import mjpeg as MJ
from openglottal_amd import synth

pytestmark = pytest.mark.gpu

FEATS = (4, 8, 16, 32)
N = 12
hit = lambda x, y: [[x, y, x + 30.0, y + 24.0, 0.9]]
SCRIPT = [hit(20 + i, 15 + i) for i in range(3)] + [[]] * 5 + [hit(31 + i, 26) for i in range(4)]
SHAPES = ((256, 256), (K.H, K.W))


def scripted():
    calls = {"i": 0}

    def backend(frame, conf):
        d = [x for x in SCRIPT[calls["i"]] if x[4] >= conf]
        calls["i"] += 1
        return (np.array([x[:4] for x in d], np.float32).reshape(-1, 4), np.array([x[4] for x in d], np.float32))

    return og.TemporalDetector(backend)


@pytest.fixture(scope="module")
def model():
    m = og.UNet(1, 1, FEATS)
    m.load_state_dict(synth.make_unet_state_dict(FEATS, seed=11, head_scale=3.0, head_bias=0.5))
    m.to("cuda:0").eval()
    m.set_chunk(4)
    return m


def video(H, W):
    v = np.random.RandomState(H + 3 * W).randint(0, 256, (N, H, W, 3), dtype=np.uint8)
    v //= 2                                                               # (room for the fill's + 102)
    v[:, :, : W // 2] = v[:, :1, : W // 2]                                # half of it smooth along y: runs of zeros, EOB
    return v


@pytest.mark.parametrize("H,W", SHAPES)
def test_the_files_are_the_host_twins_encoding_of_run_pipelines_frames(model, monkeypatch, H, W):
    monkeypatch.setattr(F, "BLOCK", 8)                                    # two blocks: 8 frames and 4
    v = video(H, W)
    frames, wave = I.run_pipeline(v, scripted(), "unet", model, "cuda:0")
    assert wave.max() > 0 and not np.array_equal(frames, v)
    enc = MJ.Mjpeg(quality=80, chunk=3)
    blocks = list(I.iter_pipeline_mjpeg(v, scripted(), "unet", model, "cuda:0", encoder=enc))
    assert [len(b[1]) for b in blocks] == [8, 4] and all(len(b) == 3 for b in blocks)
    files = [j for blob, sizes, _ in blocks for j in MJ.split(blob, sizes)]
    assert files == [MJ.encode_host(f, 80) for f in frames]
    area = np.concatenate([b[2] for b in blocks])
    assert area.dtype == np.float64 and np.array_equal(area, wave)
    # with the frames asked for, they are run_pipeline's
    got = list(I.iter_pipeline_mjpeg(v, None, "unet-only", model, "cuda:0", overlay_style="contour", encoder=enc, frames=True))
    ref, ref_wave = I.run_pipeline(v, None, "unet-only", model, "cuda:0", overlay_style="contour")
    assert np.array_equal(np.concatenate([g[3] for g in got]), ref) and np.array_equal(np.concatenate([g[2] for g in got]), ref_wave)
    assert [j for blob, sizes, _, _ in got for j in MJ.split(blob, sizes)] == [MJ.encode_host(f, 80) for f in ref]


def listing(d):
    return sorted(os.listdir(d))


def test_cli_infer_writes_an_avi_of_those_bytes_and_leaves_the_rest_alone(tmp_path, capsys, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)                         # no OpenCV, wherever this runs: `import cv2` raises ImportError
    feats = (32, 64, 128, 256)
    sd = synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5)
    torch.save(synth.state_dict_to_torch(sd), tmp_path / "unet.pt")
    H, W = 72, 100
    v = video(H, W)
    os.makedirs(tmp_path / "in")
    np.save(tmp_path / "in" / "clip.npy", v)
    base = ["infer", "--input", str(tmp_path / "in"), "--mode", "npy", "--pipeline", "unet-only", "--unet-weights", str(tmp_path / "unet.pt")]

    assert cli.main(base + ["--output-dir", str(tmp_path / "plain")]) == 0
    out = capsys.readouterr().out
    assert "OpenCV is not importable: annotated videos are written as <stem>_out.npy" in out
    assert listing(tmp_path / "plain") == ["clip_out.npy", "features.csv"]            # what it held before this flag existed
    frames = np.load(tmp_path / "plain" / "clip_out.npy")

    assert cli.main(base + ["--output-dir", str(tmp_path / "both"), "--avi", "device", "--jpeg-quality", "90"]) == 0
    out = capsys.readouterr().out
    assert "OpenCV is not importable" not in out and "clip_out.avi" in out
    assert listing(tmp_path / "both") == ["clip_out.avi", "clip_out.npy", "features.csv"]
    assert np.array_equal(np.load(tmp_path / "both" / "clip_out.npy"), frames)
    data = open(tmp_path / "both" / "clip_out.avi", "rb").read()
    top = MC.riff_walk(data, 0, len(data))
    assert len(top) == 1 and [k[0] for k in top[0][3]] == [b"hdrl", b"movi", b"idx1"]
    hdrl, movi, idx1 = top[0][3]
    avih = struct.unpack_from("<14I", data, hdrl[3][0][1])
    assert avih[0] == 40000 and avih[4] == N and avih[8:10] == (W, H)                 # 25 fps
    chunks = [data[at:at + n] for cc, at, n, _ in movi[3]]
    assert chunks == [MJ.encode_host(f, 90) for f in frames]
    assert idx1[2] == 16 * N
    got = F.load_frames_bgr(str(tmp_path / "both" / "clip_out.avi"))
    assert len(got) == N and min(MC.psnr(g, f) for g, f in zip(got, frames)) > 25

    assert cli.main(base + ["--output-dir", str(tmp_path / "avi"), "--avi", "device", "--jpeg-quality", "90", "--no-npy"]) == 0
    capsys.readouterr()
    assert listing(tmp_path / "avi") == ["clip_out.avi", "features.csv"]
    assert open(tmp_path / "avi" / "clip_out.avi", "rb").read() == data
    rows = [list(csv.reader(open(tmp_path / d / "features.csv", newline=""))) for d in ("plain", "both", "avi")]
    assert rows[0] == rows[1] == rows[2] and len(rows[0]) == 2
