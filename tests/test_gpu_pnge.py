"""-m gpu: the device PNG encoder (include_enc/openglottal_hip_pnge.h) against its host twin, byte for byte, on the whole case list of
tests/pnge_cases.py.  Every case goes up as a batch of seven frames at chunk 3, so each call has three micro-batches and both pinned
slots turn over; one handle per (C, S).  The resident entry gives the streamed entry's bytes, and the device's files go back through
the device decoder to the pixels they were made from."""
import numpy as np
import pytest

import pnge_cases as EC
from openglottal_amd import png as P

pytestmark = pytest.mark.gpu

GROUPS = sorted({(f.shape[2], S) for _, f, S in EC.cases()})


def _ids(C, S):
    return [cid for cid, f, s in EC.cases() if f.shape[2] == C and s == S]


@pytest.mark.parametrize("C,S", GROUPS)
def test_device_bytes_and_sizes_equal_the_twins(C, S):
    e = P.PngEncoder(chunk=3, segment=S)
    for cid in _ids(C, S):
        want = EC.host_files(cid)
        blob, sizes = e.encode(EC.batch(cid))
        assert sizes.tolist() == [len(f) for f in want], cid
        assert blob.tobytes() == b"".join(want), cid


@pytest.mark.parametrize("cid", ["runs-c1-s64", "filters-c3-s64", "noise-c1-s256", "fibonacci-c1-s32768", "two-segments-181x182-c3-s32768",
                                 "synth0-c1-s32768", "zeros-256-c1-s32768"])
def test_resident_entry_equals_streamed_entry(cid):
    import torch

    frames = EC.batch(cid)
    B, H, W, C = frames.shape
    e = P.PngEncoder(chunk=3, segment=EC.by_id(cid)[2])
    blob, sizes, total = e.encode_resident(torch.from_numpy(frames).cuda(), B, H, W, C)
    e.sync()
    want = EC.host_files(cid)
    assert int(total[0]) == sum(len(f) for f in want) and sizes.cpu().tolist() == [len(f) for f in want]
    assert blob[:int(total[0])].cpu().numpy().tobytes() == b"".join(want)


@pytest.mark.parametrize("C", [1, 3])
def test_device_files_decode_on_the_device_to_the_input_pixels(C):
    e, d = P.PngEncoder(chunk=3), P.PngDecoder(chunk=3)
    for cid in (f"two-segments-181x182-c{C}-s32768", f"synth0-c{C}-s32768", f"filters-c{C}-s32768", f"h1-c{C}-s32768"):
        frames = EC.batch(cid)
        back = d.decode(e.files(frames), C)
        assert isinstance(back, np.ndarray) and np.array_equal(back, frames), cid


def test_b0_and_a_handle_reused_across_shapes_and_segments():
    e = P.PngEncoder(chunk=2, segment=64)
    blob, sizes = e.encode(np.zeros((0, 4, 4, 1), np.uint8))
    assert blob.size == 0 and sizes.size == 0
    for cid in ("seam-rows-c1-s64", "noise-c3-s256", "h1-c1-s32768", "seam-rows-c3-s64"):
        e.set_segment(EC.by_id(cid)[2])
        assert b"".join(e.files(EC.batch(cid))) == b"".join(EC.host_files(cid)), cid


def test_cli_infer_png_device_against_pillow(tmp_path, capsys, monkeypatch):
    """`cli infer --frames png --png device` on a 12-frame 64 x 96 clip: the names of `--png pillow`, the same pixels after decoding,
    the twin's bytes; with and without `--avi device`, and with `--no-npy` no raw frame is written."""
    import io
    import os
    import sys

    import torch
    from PIL import Image

    from openglottal_amd import cli, synth

    monkeypatch.setitem(sys.modules, "cv2", None)
    feats = (32, 64, 128, 256)
    torch.save(synth.state_dict_to_torch(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5)), tmp_path / "unet.pt")
    v = np.random.RandomState(7).randint(0, 256, (12, 64, 96, 3), dtype=np.uint8) // 2
    v[:, :, :48] = v[:, :1, :48]
    os.makedirs(tmp_path / "in")
    np.save(tmp_path / "in" / "clip.npy", v)
    base = ["infer", "--input", str(tmp_path / "in"), "--mode", "npy", "--pipeline", "unet-only", "--unet-weights", str(tmp_path / "unet.pt"),
            "--frames", "png"]
    runs = {"pillow": [], "device": ["--png", "device"], "device-avi": ["--png", "device", "--avi", "device"],
            "device-avi-no-npy": ["--png", "device", "--avi", "device", "--no-npy"]}
    for name, extra in runs.items():
        assert cli.main(base + ["--output-dir", str(tmp_path / name)] + extra) == 0
    capsys.readouterr()
    names = sorted(os.listdir(tmp_path / "pillow" / "clip_out"))
    assert names == [f"{i:06d}.png" for i in range(12)]
    frames = np.load(tmp_path / "pillow" / "clip_out.npy")
    for name in list(runs)[1:]:
        d = tmp_path / name / "clip_out"
        assert sorted(os.listdir(d)) == names, name
        for i, n in enumerate(names):
            data = open(d / n, "rb").read()
            a, b = np.asarray(Image.open(io.BytesIO(data))), np.asarray(Image.open(tmp_path / "pillow" / "clip_out" / n))
            assert np.array_equal(a, b) and np.array_equal(a[..., ::-1], frames[i]), (name, n)
            assert data == P.encode_host(frames[i]), (name, n)
    assert sorted(os.listdir(tmp_path / "device")) == ["clip_out", "clip_out.npy", "features.csv"]
    assert sorted(os.listdir(tmp_path / "device-avi")) == ["clip_out", "clip_out.avi", "clip_out.npy", "features.csv"]
    assert sorted(os.listdir(tmp_path / "device-avi-no-npy")) == ["clip_out", "clip_out.avi", "features.csv"]
    assert np.array_equal(np.load(tmp_path / "device" / "clip_out.npy"), frames)
    assert open(tmp_path / "device-avi" / "clip_out.avi", "rb").read() == open(tmp_path / "device-avi-no-npy" / "clip_out.avi", "rb").read()
    feats_csv = [open(tmp_path / n / "features.csv").read() for n in runs]
    assert len(set(feats_csv)) == 1
