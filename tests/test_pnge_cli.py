"""`cli infer --png device` and `cli crop-cache`: what the argument parser refuses, with the reason, before anything is loaded.  No GPU."""
import pytest

from openglottal_amd import cli

BASE = ["infer", "--input", "nowhere", "--mode", "npy", "--pipeline", "unet-only", "--unet-weights", "none.pt"]


def refused(argv, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_png_device_needs_frames_png(capsys):
    assert "--png device goes with --frames png only" in refused(BASE + ["--png", "device"], capsys)


def test_label_is_refused_with_png_device_and_says_why(capsys):
    err = refused(BASE + ["--frames", "png", "--png", "device", "--label"], capsys)
    assert "--label draws on the host" in err and "--png device" in err


def test_no_npy_with_pillow_pngs_is_still_refused_and_points_to_the_device_coder(capsys):
    err = refused(BASE + ["--frames", "png", "--avi", "device", "--no-npy"], capsys)
    assert "--frames png needs the annotated frames on the host" in err and "--png device" in err


def test_crop_cache_refuses_bad_arguments(capsys, tmp_path):
    base = ["crop-cache", "--images", str(tmp_path), "--labels", str(tmp_path), "--out", str(tmp_path / "cache"), "--split", "train"]
    assert "--yolo-weights" in refused(base, capsys)                          # roi yolo is the default and needs the detector
    assert "invalid choice" in refused(base + ["--roi", "box"], capsys)
    assert "--crop-size" in refused(base + ["--roi", "gt", "--crop-size", "0"], capsys)
