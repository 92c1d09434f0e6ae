"""`cli infer --mode images --decode device|auto` and `cli run <dir> --decode` on directories of .png frames, without a device: the
all-.png directory takes the PNG decoder, a directory that mixes .jpg and .png keeps the behaviour tests/test_mjpd_cli.py pins, and
`--decode host` (the default) is untouched."""
import argparse
import os

import numpy as np
import pytest
from PIL import Image

from openglottal_amd import cli
from openglottal_amd import png as P
from openglottal_amd._lib import OpenGlottalHipError


def _parser():
    ap = argparse.ArgumentParser(prog="openglottal_amd")
    sub = ap.add_subparsers(dest="cmd", required=True)
    cli.add_infer_parser(sub)
    return ap


def _seq(path, sizes):
    os.makedirs(path)
    rs = np.random.RandomState(0)
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(rs.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(path / f"{i:03d}.png")


def test_a_png_directory_takes_the_device_decoder(tmp_path, capsys):
    _seq(tmp_path / "seq", [(24, 40)] * 3)
    (tmp_path / "seq" / "notes.txt").write_text("x")
    for mode in ("device", "auto"):
        a = _parser().parse_args(["infer", "--input", str(tmp_path / "seq"), "--mode", "images", "--decode", mode])
        jobs = list(cli._infer_jobs(a))
        assert len(jobs) == 1 and jobs[0][0] == "seq" and isinstance(jobs[0][1], P.CompressedImages)
        v = jobs[0][1]
        assert (len(v), v.H, v.W) == (3, 24, 40) and isinstance(v.decoder, P.PngDecoder)
        want = np.ascontiguousarray(np.asarray(Image.open(tmp_path / "seq" / "001.png").convert("RGB"))[..., ::-1])
        assert np.array_equal(v[1], want)                                     # (one frame by the host twin: a size or a seed frame)
    assert capsys.readouterr().err == ""
    a = _parser().parse_args(["infer", "--input", str(tmp_path / "seq"), "--mode", "images"])
    jobs = list(cli._infer_jobs(a))
    assert a.decode == "host" and isinstance(jobs[0][1], list) and len(jobs[0][1]) == 3      # the default: today's Pillow loop


def test_sizes_that_differ_and_refused_frames(tmp_path, capsys):
    _seq(tmp_path / "mixed", [(24, 40), (24, 41)])
    a = _parser().parse_args(["infer", "--input", str(tmp_path / "mixed"), "--mode", "images", "--decode", "device"])
    with pytest.raises(OpenGlottalHipError, match="different sizes"):
        list(cli._infer_jobs(a))
    a = _parser().parse_args(["infer", "--input", str(tmp_path / "mixed"), "--mode", "images", "--decode", "auto"])
    jobs = list(cli._infer_jobs(a))
    err = capsys.readouterr().err
    assert isinstance(jobs[0][1], list) and len(jobs[0][1]) == 2 and err.count("\n") == 1 and "--decode auto" in err and "host" in err
    os.makedirs(tmp_path / "deep")
    Image.fromarray(np.zeros((4, 4), np.uint16)).save(tmp_path / "deep" / "0.png")
    assert P.open_compressed(str(tmp_path / "deep"), "auto") is None and "16-bit" in capsys.readouterr().err
    with pytest.raises(OpenGlottalHipError, match="16-bit"):
        P.open_compressed(str(tmp_path / "deep"), "device")


def test_run_routes_a_png_directory_to_the_png_decoder(tmp_path, monkeypatch):
    _seq(tmp_path / "seq", [(8, 8)] * 2)
    seen = []

    class Fake:
        def frames_host(self):
            return "frames"

    monkeypatch.setattr(P, "open_compressed", lambda path, mode: seen.append((path, mode)) or Fake())
    a = argparse.Namespace(video=str(tmp_path / "seq"), decode="device", decode_split="off")
    assert cli._decoded_on_device(a) == "frames" and seen == [(str(tmp_path / "seq"), "device")]
    (tmp_path / "seq" / "x.jpg").write_bytes(b"")                             # no longer .png only: the JPEG path, as before
    with pytest.raises(OpenGlottalHipError):
        cli._decoded_on_device(a)
    assert len(seen) == 1
    assert "directory of .png frames" in _parser()._subparsers._group_actions[0].choices["infer"].format_help().replace("\n", " ").replace("  ", " ")
