"""`cli infer --decode` and `cli run --decode` without a device: the flag, its default (`host`: today's path), its refusals, the one
stderr line of `--decode auto`, and the RIFF walk that hands the compressed frames over."""
import argparse
import io
import os

import numpy as np
import pytest
from PIL import Image

import mjpd_cases as DC
from openglottal_amd import cli
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import OpenGlottalHipError


def _parser():
    ap = argparse.ArgumentParser(prog="openglottal_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    cli.add_infer_parser(sub)
    return ap


def test_the_flag_and_the_unchanged_defaults():
    a = _parser().parse_args(["infer", "--input", "videos"])
    assert a.decode == "host"
    assert (a.avi, a.jpeg_quality, a.no_npy, a.mode, a.pipeline, a.output_dir, a.device) == ("opencv", 75, False, "avi", "unet", "results", "cuda")
    for v in ("device", "auto", "host"):
        assert _parser().parse_args(["infer", "--input", "d", "--decode", v]).decode == v
    with pytest.raises(SystemExit):
        _parser().parse_args(["infer", "--input", "d", "--decode", "gpu"])
    help_text = _parser()._subparsers._group_actions[0].choices["infer"].format_help()
    assert "--decode" in help_text and "baseline JPEG" in help_text


def test_refusals_come_before_anything_is_loaded(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["infer", "--input", "d", "--mode", "npy", "--pipeline", "unet-only", "--unet-weights", "u.pt", "--decode", "device"])
    assert e.value.code == 2 and "compressed input" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(["run", "clip.npy", "--pipeline", "guided-vft", "--yolo-weights", "y.npz", "--decode", "device", "--bogus"])
    assert e.value.code == 2


def _avi(path, files, W, H):
    with MJ.AviWriter(str(path), W, H) as w:
        w.write(np.frombuffer(b"".join(files), np.uint8), [len(f) for f in files])


def test_the_riff_walk_hands_over_the_compressed_frames(tmp_path):
    files = [MJ.encode_host(DC.noise(24, 40, s), 75) for s in range(5)]
    _avi(tmp_path / "clip.avi", files, 40, 24)
    assert MJ.jpeg_files(str(tmp_path / "clip.avi")) == files
    os.makedirs(tmp_path / "seq")
    for i, f in enumerate(files):
        (tmp_path / "seq" / f"{i:03d}.jpg").write_bytes(f)
    (tmp_path / "seq" / "notes.txt").write_text("x")
    assert MJ.jpeg_files(str(tmp_path / "seq")) == files
    with pytest.raises(OpenGlottalHipError, match="no .jpg"):
        os.makedirs(tmp_path / "empty")
        MJ.jpeg_files(str(tmp_path / "empty"))


def test_decode_auto_falls_back_for_a_directory_that_is_not_all_jpeg(tmp_path, capsys):
    """`--mode images --decode auto` on a directory that also holds a .png: the host loop, one line on stderr; `device` refuses."""
    os.makedirs(tmp_path / "seq")
    (tmp_path / "seq" / "000.jpg").write_bytes(MJ.encode_host(DC.noise(24, 40), 75))
    Image.fromarray(DC.noise(24, 40)).save(tmp_path / "seq" / "001.png")
    ap = _parser()
    a = ap.parse_args(["infer", "--input", str(tmp_path / "seq"), "--mode", "images", "--decode", "auto"])
    jobs = list(cli._infer_jobs(a))
    err = capsys.readouterr().err
    assert len(jobs) == 1 and isinstance(jobs[0][1], list) and len(jobs[0][1]) == 2 and jobs[0][1][0].shape == (24, 40, 3)
    assert err.count("\n") == 1 and "--decode auto" in err and "host" in err
    a = ap.parse_args(["infer", "--input", str(tmp_path / "seq"), "--mode", "images", "--decode", "device"])
    with pytest.raises(SystemExit, match=".jpg frames only"):
        list(cli._infer_jobs(a))


def test_run_checks_its_arguments_before_it_decodes(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(cli, "_decoded_on_device", lambda a: pytest.fail("decoded before the argument checks"))
    for argv, word in ((["--pipeline", "unet", "--unet-weights", "u.pt"], "--yolo-weights"),
                       (["--pipeline", "yolo-crop+unet", "--yolo-weights", "y.npz"], "--crop-weights"),
                       (["--pipeline", "unet-only"], "--unet-weights"), (["--pipeline", "guided-vft"], "--yolo-weights")):
        with pytest.raises(SystemExit) as e:
            cli.main(["run", str(tmp_path / "clip.avi"), "--decode", "device"] + argv)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_decode_auto_says_once_why_it_takes_the_host_loop(tmp_path, capsys):
    b = io.BytesIO()
    Image.fromarray(DC.noise(24, 40)).save(b, "JPEG", progressive=True)
    _avi(tmp_path / "prog.avi", [b.getvalue()] * 2, 40, 24)
    assert MJ.open_compressed(str(tmp_path / "prog.avi"), "auto") is None
    err = capsys.readouterr().err
    assert err.count("\n") == 1 and "--decode auto" in err and "progressive" in err and "host" in err
    with pytest.raises(OpenGlottalHipError, match="progressive"):
        MJ.open_compressed(str(tmp_path / "prog.avi"), "device")
