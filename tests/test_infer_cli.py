"""`python -m openglottal_amd.cli infer` without a device: the argparse surface (the reference's flag names), the refusal of `vft`,
the formatting of features.csv from scripted waveforms (f0 None and a silent one among them), and the block-wise .npy writer."""
import argparse
import csv

import numpy as np
import pytest

from openglottal_amd import cli
from openglottal_amd import infer as I
from openglottal_amd._lib import OpenGlottalHipError
from openglottal_amd.features import _kinematic_features


def _parser():
    ap = argparse.ArgumentParser(prog="openglottal_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    cli.add_infer_parser(sub)
    return ap


def test_the_argparse_surface():
    a = _parser().parse_args(["infer", "--input", "videos"])
    assert (a.input, a.mode, a.pipeline, a.output_dir, a.capture_fps, a.max_hold_frames, a.overlay_style, a.device) == \
        ("videos", "avi", "unet", "results", 4000.0, 3, "fill", "cuda")
    assert a.yolo_weights is None and a.unet_weights is None and a.crop_weights is None
    assert a.label is False and a.frames == "npy" and a.precision == "f32" and a.detector_precision == "f32"
    a = _parser().parse_args(["infer", "--input", "d", "--mode", "npy", "--pipeline", "yolo-crop+unet", "--yolo-weights", "y.npz",
                              "--unet-weights", "u.pt", "--crop-weights", "c.pt", "--output-dir", "o", "--capture-fps", "2000",
                              "--max-hold-frames", "0", "--overlay-style", "contour", "--device", "cuda:1", "--frames", "png", "--label",
                              "--precision", "f16", "--detector-precision", "f16"])
    assert (a.mode, a.pipeline, a.yolo_weights, a.unet_weights, a.crop_weights, a.output_dir) == ("npy", "yolo-crop+unet", "y.npz", "u.pt", "c.pt", "o")
    assert (a.capture_fps, a.max_hold_frames, a.overlay_style, a.device, a.frames, a.label) == (2000.0, 0, "contour", "cuda:1", "png", True)
    assert (a.precision, a.detector_precision) == ("f16", "f16")
    for mode in ("avi", "images", "npy"):
        assert _parser().parse_args(["infer", "--input", "d", "--mode", mode]).mode == mode
    for bad in (["--mode", "mp4"], ["--overlay-style", "solid"], ["--pipeline", "otsu"], []):
        with pytest.raises(SystemExit):
            _parser().parse_args(["infer"] + (bad if bad else []) + (["--input", "d"] if bad else []))
    help_text = _parser()._subparsers._group_actions[0].choices["infer"].format_help()
    assert "NOT" in help_text and "OpenCV" in help_text and "Hershey" in help_text       # --label says whose glyphs these are not


def test_vft_is_refused_with_the_sentence_run_uses(capsys):
    for argv in (["infer", "--input", "d", "--pipeline", "vft", "--yolo-weights", "y.npz"], ["run", "v.npy", "--pipeline", "vft"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
        assert "Gaussian-blurred f32 motion map" in capsys.readouterr().err
    with pytest.raises(OpenGlottalHipError, match="Gaussian-blurred f32 motion map"):
        I.run_pipeline(np.zeros((2, 8, 8, 3), np.uint8), None, "vft", None)
    with pytest.raises(OpenGlottalHipError):
        I.run_pipeline(np.zeros((2, 8, 8, 3), np.uint8), None, "otsu", None)


def test_required_weights_are_asked_for_before_anything_is_loaded(capsys):
    for argv, word in ((["--pipeline", "unet"], "--unet-weights"), (["--pipeline", "unet-only"], "--unet-weights"),
                       (["--pipeline", "yolo-crop+unet", "--yolo-weights", "y"], "--crop-weights"),
                       (["--pipeline", "guided-vft"], "--yolo-weights"), (["--pipeline", "unet", "--unet-weights", "u"], "--yolo-weights")):
        with pytest.raises(SystemExit) as e:
            cli.main(["infer", "--input", "d"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_features_csv_formatting(tmp_path):
    t = np.arange(64)
    voiced = 500.0 + 300.0 * np.sin(2 * np.pi * t / 8.0)                  # eight frames a cycle: f0 = 0.125 cycles per frame
    drift = np.linspace(10.0, 90.0, 64)                                   # the peak sits in the first bin: f0 None
    assert _kinematic_features(drift)["f0"] is None and _kinematic_features(voiced)["f0"] == 0.125
    rows = [I.features_row("voiced", voiced, 4000.0), I.features_row("drift", drift, 4000.0), I.features_row("silent", np.zeros(20), 4000.0)]
    path = tmp_path / "features.csv"
    I.write_features_csv(str(path), rows)
    with open(path, newline="") as f:
        got = list(csv.reader(f))
    assert got[0] == ["source", "area_mean", "area_std", "area_range", "open_quotient", "f0", "periodicity", "cv"]
    k = _kinematic_features(voiced)
    assert got[1] == ["voiced"] + [f"{k[c]:.4f}" if c != "f0" else "500.0000" for c in I.FEATURE_COLS]     # 0.125 * 4000 Hz
    assert got[1][1] == "500.0000" and all(len(c.split(".")[1]) == 4 for c in got[1][1:])
    assert got[2][0] == "drift" and got[2][5] == "" and all(c != "" for i, c in enumerate(got[2]) if i != 5)  # f0 None: an empty cell
    assert got[3] == ["silent"] + [""] * 7
    assert I.features_row("v", voiced, 2000.0)["f0"] == "250.0000"


def test_the_npy_writer_block_by_block_equals_np_save(tmp_path):
    rs = np.random.RandomState(0)
    video = rs.randint(0, 256, (11, 6, 7, 3), dtype=np.uint8)
    one, blocks = tmp_path / "one.npy", tmp_path / "blocks.npy"
    np.save(one, video)
    w = I.NpyWriter(str(blocks), len(video))
    for lo in (0, 4, 8):
        w.write(video[lo:lo + 4])                                         # the last block is ragged
    w.close()
    assert open(one, "rb").read() == open(blocks, "rb").read()
    assert np.array_equal(np.load(blocks), video)
    w = I.NpyWriter(str(tmp_path / "short.npy"), 5)
    w.write(video[:3])
    with pytest.raises(OpenGlottalHipError):
        w.close()


def test_the_png_writer_and_the_host_label(tmp_path):
    from PIL import Image

    from openglottal_amd.overlay import label_host

    f = np.zeros((2, 24, 64, 3), np.uint8)
    f[..., 0] = 200                                                       # blue in BGR
    I.write_pngs(str(tmp_path / "v_out"), 7, f)
    img = np.asarray(Image.open(tmp_path / "v_out" / "000008.png"))
    assert img.shape == (24, 64, 3) and tuple(img[0, 0]) == (0, 0, 200)   # RGB on disk
    out = label_host(f[0], 1234.7)
    assert out.shape == f[0].shape and not np.array_equal(out, f[0]) and (f[0][..., 0] == 200).all()      # a fresh array with white text
    assert (out[20:] == f[0][20:]).all() and (out.min(-1) > 100).any()                     # (the font may be anti-aliased)
