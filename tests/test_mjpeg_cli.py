"""`python -m openglottal_amd.cli infer --avi device` without a device: the new flags, their refusals, and the defaults of every
flag that was there before."""
import argparse

import pytest

from openglottal_amd import cli


def _parser():
    ap = argparse.ArgumentParser(prog="openglottal_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    cli.add_infer_parser(sub)
    return ap


def test_the_new_flags_and_the_unchanged_defaults():
    a = _parser().parse_args(["infer", "--input", "videos"])
    assert (a.avi, a.jpeg_quality, a.no_npy) == ("opencv", 75, False)
    assert (a.input, a.mode, a.pipeline, a.output_dir, a.capture_fps, a.max_hold_frames, a.overlay_style, a.device) == \
        ("videos", "avi", "unet", "results", 4000.0, 3, "fill", "cuda")
    assert a.label is False and a.frames == "npy" and a.precision == "f32" and a.detector_precision == "f32" and a.skip_unboxed is False
    a = _parser().parse_args(["infer", "--input", "d", "--avi", "device", "--jpeg-quality", "90", "--no-npy"])
    assert (a.avi, a.jpeg_quality, a.no_npy) == ("device", 90, True)
    with pytest.raises(SystemExit):
        _parser().parse_args(["infer", "--input", "d", "--avi", "host"])
    with pytest.raises(SystemExit):
        _parser().parse_args(["infer", "--input", "d", "--jpeg-quality", "high"])
    help_text = _parser()._subparsers._group_actions[0].choices["infer"].format_help()
    assert "--avi" in help_text and "Motion-JPEG" in help_text and "--no-npy" in help_text


BASE = ["infer", "--input", "d", "--pipeline", "unet-only", "--unet-weights", "u.pt"]


@pytest.mark.parametrize("argv,words", [
    (["--avi", "device", "--label"], ("--label", "on the host")),
    (["--avi", "device", "--jpeg-quality", "0"], ("--jpeg-quality", "1..100")),
    (["--avi", "device", "--jpeg-quality", "101"], ("--jpeg-quality", "1..100")),
    (["--no-npy"], ("--no-npy", "--avi device")),
    (["--avi", "device", "--no-npy", "--frames", "png"], ("--frames png", "--no-npy")),
])
def test_refusals_come_before_anything_is_loaded(capsys, argv, words):
    with pytest.raises(SystemExit) as e:
        cli.main(BASE + argv)                                             # (u.pt does not exist: nothing may try to open it)
    err = capsys.readouterr().err
    assert e.value.code == 2 and all(w in err for w in words), err


def test_vft_stays_refused_with_the_device_avi(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["infer", "--input", "d", "--pipeline", "vft", "--yolo-weights", "y.npz", "--avi", "device"])
    assert e.value.code == 2 and "Gaussian-blurred f32 motion map" in capsys.readouterr().err
