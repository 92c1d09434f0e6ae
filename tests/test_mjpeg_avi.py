"""`mjpeg.AviWriter`, `mjpeg.read_avi_mjpeg` and `features.load_frames_bgr` on files made of the host twin's JPEGs: the RIFF walk of
tests/mjpeg_cases.py checks every size, pad, index entry and header field.  No GPU, no OpenCV."""
import struct
import sys

import numpy as np
import pytest

import mjpeg_cases as MC
from openglottal_amd import features as F
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import OpenGlottalHipError


walk = MC.riff_walk


def video():
    """7 frames of 40 x 56 whose files have odd and even lengths"""
    c = MC.BY_ID["batch7"]
    files = MC.host_files("batch7")
    assert any(len(j) % 2 for j in files) and any(len(j) % 2 == 0 for j in files)
    return c.frames, files


def write(path, files, blocks=((0, 3), (3, 7)), fps=25.0, H=40, W=56):
    w = MJ.AviWriter(str(path), W, H, fps)
    for lo, hi in blocks:
        w.write(np.frombuffer(b"".join(files[lo:hi]), np.uint8), np.array([len(j) for j in files[lo:hi]], np.int32))
    w.close()
    w.close()                                                             # idempotent
    return open(path, "rb").read()


def test_the_riff_structure_adds_up(tmp_path):
    frames, files = video()
    data = write(tmp_path / "v.avi", files)
    assert data[:4] == b"RIFF" and struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and data[8:12] == b"AVI "
    top = walk(data, 0, len(data))
    assert len(top) == 1 and top[0][0] == b"AVI "
    kids = top[0][3]
    assert [k[0] for k in kids] == [b"hdrl", b"movi", b"idx1"]
    hdrl, movi, idx1 = kids
    assert [k[0] for k in hdrl[3]] == [b"avih", b"strl"] and [k[0] for k in hdrl[3][1][3]] == [b"strh", b"strf"]
    avih = struct.unpack_from("<14I", data, hdrl[3][0][1])
    assert hdrl[3][0][2] == 56 and avih[0] == 40000 and avih[3] & 0x10 and avih[4] == 7 and avih[6] == 1 and avih[8:10] == (56, 40)
    assert avih[7] == max(len(j) for j in files)
    strh_at = hdrl[3][1][3][0][1]
    assert data[strh_at:strh_at + 8] == b"vidsMJPG"
    scale, rate, start, length = struct.unpack_from("<4I", data, strh_at + 20)
    assert rate / scale == 25.0 and start == 0 and length == 7
    assert struct.unpack_from("<4H", data, strh_at + 48) == (0, 0, 56, 40)
    strf = struct.unpack_from("<IiiHH4sI", data, hdrl[3][1][3][1][1])
    assert strf == (40, 56, 40, 1, 24, b"MJPG", 56 * 40 * 3)
    # movi: one 00dc chunk per frame, the very bytes, odd ones padded with a zero
    chunks = movi[3]
    assert [c[0] for c in chunks] == [b"00dc"] * 7
    for (cc, at, n, _), j in zip(chunks, files):
        assert data[at:at + n] == j
        if n & 1:
            assert data[at + n] == 0
    # idx1: 16 bytes per frame; offsets from the "movi" fourcc point at the chunk headers
    assert idx1[2] == 16 * 7
    movi_fourcc = movi[1]
    for i, (cc, at, n, _) in enumerate(chunks):
        ck, flags, off, size = struct.unpack_from("<4sIII", data, idx1[1] + 16 * i)
        assert (ck, flags, size) == (b"00dc", 0x10, n)
        assert movi_fourcc + off == at - 8 and data[movi_fourcc + off:movi_fourcc + off + 4] == b"00dc"


def test_reading_back(tmp_path):
    frames, files = video()
    write(tmp_path / "v.avi", files, blocks=((0, 7),), fps=30.0)
    got = MJ.read_avi_mjpeg(str(tmp_path / "v.avi"))
    assert len(got) == 7
    for g, j, f in zip(got, files, frames):
        assert g.shape == f.shape and g.dtype == np.uint8 and np.array_equal(g, MC.pillow_decode(j))
    handler, chunks = MJ.avi_stream(str(tmp_path / "v.avi"))
    assert handler == b"MJPG" and list(chunks) == list(files)


def test_load_frames_bgr_reads_it_without_opencv(tmp_path, monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)                         # `import cv2` raises ImportError, wherever this runs
    with pytest.raises(ImportError):
        import cv2  # noqa: F401
    frames, files = video()
    write(tmp_path / "v.avi", files)
    got = F.load_frames_bgr(str(tmp_path / "v.avi"))
    assert len(got) == 7 and all(g.shape == (40, 56, 3) and g.dtype == np.uint8 for g in got)
    assert np.array_equal(got[2], MC.pillow_decode(files[2]))
    assert MC.psnr(got[2], frames[2]) > 30
    # every other codec is still the error it was
    data = bytearray(open(tmp_path / "v.avi", "rb").read())
    at = data.index(b"vidsMJPG")
    data[at + 4:at + 8] = b"XVID"
    (tmp_path / "x.avi").write_bytes(bytes(data))
    with pytest.raises(OpenGlottalHipError, match="needs OpenCV"):
        F.load_frames_bgr(str(tmp_path / "x.avi"))
    with pytest.raises(OpenGlottalHipError, match="MJPG"):
        MJ.read_avi_mjpeg(str(tmp_path / "x.avi"))
    (tmp_path / "junk.avi").write_bytes(b"not a riff file at all")
    with pytest.raises(OpenGlottalHipError):
        F.load_frames_bgr(str(tmp_path / "junk.avi"))
    assert F.load_frames_bgr(str(tmp_path / "absent.avi")) == []


def test_a_file_that_would_pass_the_limit_is_refused_before_the_frame_is_written(tmp_path):
    frames, files = video()
    assert MJ.RIFF_LIMIT == 2 ** 31 - 1
    whole = len(write(tmp_path / "whole.avi", files))
    w = MJ.AviWriter(str(tmp_path / "v.avi"), 56, 40, 25.0)
    assert w.limit == MJ.RIFF_LIMIT
    w.limit = whole - 1                                                   # (patched: not a 2 GB file)
    blob = lambda js: (np.frombuffer(b"".join(js), np.uint8), np.array([len(j) for j in js], np.int32))
    w.write(*blob(files[:6]))
    with pytest.raises(OpenGlottalHipError, match=r"frame 6 would take the file past \d+ bytes"):
        w.write(*blob(files[6:]))
    w.close()
    data = open(tmp_path / "v.avi", "rb").read()
    assert len(data) < whole and struct.unpack_from("<I", data, 4)[0] == len(data) - 8
    assert len(MJ.read_avi_mjpeg(str(tmp_path / "v.avi"))) == 6           # the six frames before it are a complete file
    w = MJ.AviWriter(str(tmp_path / "w.avi"), 56, 40, 25.0)
    w.limit = whole
    w.write(*blob(files))                                                 # exactly the limit still fits
    w.close()
    assert len(open(tmp_path / "w.avi", "rb").read()) == whole
    with pytest.raises(OpenGlottalHipError, match="add up"):
        MJ.AviWriter(str(tmp_path / "u.avi"), 56, 40).write(np.zeros(10, np.uint8), np.array([4, 4], np.int32))
