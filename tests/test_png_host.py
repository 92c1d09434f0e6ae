"""The host twin of the device PNG decoder (og_pngd_*_host, include_ext/openglottal_hip_png.h) against two other decoders: an
independent numpy unfilter over zlib.decompress (tests/png_cases.py) and Pillow.  Valid files: status 0 and the same bytes as both.
The hostile corpus: every status occurs, status 0 => Pillow's bytes, a non-zero status => every output byte 0.  No GPU."""
import collections
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_cases as PC
from openglottal_amd import png as P
from openglottal_amd._lib import OpenGlottalHipError
from openglottal_amd.utils import bgr_to_gray

VALID = PC.valid_cases()


@pytest.mark.parametrize("name", [n for n, _ in VALID])
def test_valid_files_give_the_bytes_of_two_other_decoders(name):
    f = dict(VALID)[name]
    px, st = P.decode_host(f, 3, statuses=True)
    assert st == 0 and np.array_equal(px, PC.reference(f, 3)) and np.array_equal(px, PC.pillow(f))
    g, st = P.decode_host(f, 1, statuses=True)
    assert st == 0 and np.array_equal(g, PC.reference(f, 1)) and np.array_equal(g[..., 0], bgr_to_gray(px))
    if PC.is_gray(f):
        assert np.array_equal(g, PC.pillow(f, gray=True))                    # (a colour file's gray is unpinned against cv2 and Pillow)
    z = PC.stream_of(f)
    raw, st = P.inflate_host(z, len(zlib.decompress(z)))
    assert st == 0 and raw == zlib.decompress(z)


def test_the_valid_set_holds_what_it_claims():
    names = [n for n, _ in VALID]
    assert len(set(names)) == len(names) and sum(n.startswith("pillow-") for n in names) == 4 * len(PC.FORMS)
    info = {n: P.parse(f) for n, f in VALID}
    assert {(i["ctype"], i["depth"]) for i in info.values()} == set(PC.FORMS)
    assert info["idat-1-byte"]["nidat"] == info["idat-1-byte"]["zlib_bytes"] > 20 and info["idat-0-bytes"]["nidat"] == 2 * info["idat-0-bytes"]["zlib_bytes"]
    far = info["far-match-32768"]
    assert (far["H"], far["W"], far["rb"], far["bpp"], far["raw_bytes"]) == (182, 183, 183, 1, 182 * 184)
    assert (info["stored-65535"]["raw_bytes"], info["filter-0"]["bpp"], info["filter-0-pal4"]["rb"]) == (65535, 3, 9)
    # zlib's own block types at levels 0 and 6: stored and dynamic
    first = lambda n: (PC.stream_of(dict(VALID)[n])[2] >> 1) & 3   # noqa: E731
    assert first("pillow-2-8-l0") == 0 and first("pillow-2-8-l6") == 2 and first("fixed") == 1


def test_hand_made_invalid_streams_and_refusals():
    seen = collections.Counter()
    for name, f, want in PC.hand_made_invalid():
        px, st = P.decode_host(f, 3, statuses=True)
        assert st == want, (name, st, want, P.parse(f).get("why"))
        assert (px is None) == (st == 6) and (px is None or not px.any()), name
        seen[st] += 1
    assert set(seen) == set(range(1, 8))
    why = {n: P.parse(f)["why"] for n, f, s in PC.hand_made_invalid() if s == 6}
    for name, word in (("sixteen-bit", "16-bit"), ("adam7", "Adam7"), ("rgb-at-4", "colour type 2 at depth 4"), ("bad-crc", "CRC"),
                       ("chunk-leaves-the-file", "leaves the file"), ("missing-plte", "PLTE"), ("H-0", "H or W of 0"), ("too-many-pixels", "H * W above"),
                       ("no-idat", "no IDAT"), ("no-signature", "signature")):
        assert word in why[name], (name, why[name])
    with pytest.raises(OpenGlottalHipError, match="16-bit"):
        P.decode_host(dict((n, f) for n, f, _ in PC.hand_made_invalid())["sixteen-bit"])
    with pytest.raises(OpenGlottalHipError, match="Adler"):
        P.decode_host(dict((n, f) for n, f, _ in PC.hand_made_invalid())["adler"])


def test_the_hostile_corpus():
    seen = collections.Counter()
    for f in PC.hostile_corpus():
        px, st = P.decode_host(f, 3, statuses=True)
        seen[st] += 1
        if st == 0:
            assert np.array_equal(px, PC.pillow(f))                          # one way only: the twin is stricter than Pillow
        else:
            assert px is None or not px.any()
    assert all(seen[s] > 0 for s in range(8)), seen


def test_a_palette_index_beyond_plte_is_black_as_in_pillow():
    """Pillow 12.2 gives (0, 0, 0) for an index past the table (found here, for 8-bit and 2-bit indices)"""
    pal = bytes([10, 20, 30, 40, 50, 60])
    for depth, row in ((8, bytes([0, 1, 2, 3, 255])), (2, bytes([0b00011011, 0b11000000]))):
        f = PC.assemble(1, 5, 3, depth, zlib.compress(b"\0" + row), plte=pal)
        want = [[30, 20, 10], [60, 50, 40], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
        assert PC.pillow(f)[0].tolist() == want and P.decode_host(f)[0].tolist() == want and P.parse(f)["npal"] == 2


def test_what_pillow_tolerates_and_the_twin_does_not():
    """a short stream (Pillow pads zero rows) and surplus bytes (Pillow ignores them): statuses 1 and 4"""
    rows = PC.rng_rows(4, 6, 0, 8, 1)
    raw = PC.filter_rows(rows, [0, 1, 2, 3], 1)
    short, long = PC.assemble(4, 6, 0, 8, zlib.compress(raw[:-7])), PC.assemble(4, 6, 0, 8, zlib.compress(raw + b"xy"))
    assert P.decode_host(short, statuses=True)[1] == 1 and P.decode_host(long, statuses=True)[1] == 4
    assert not PC.pillow(short)[3].any() and np.array_equal(PC.pillow(long), P.decode_host(PC.assemble(4, 6, 0, 8, zlib.compress(raw))))


def test_inflate_host_alone():
    data = bytes(np.random.default_rng(0).integers(0, 7, 5000).astype(np.uint8))
    for level in (0, 1, 6, 9):
        z = zlib.compress(data, level)
        assert P.inflate_host(z, len(data)) == (data, 0)
        assert P.inflate_host(z, len(data) - 1)[1] == 4 and P.inflate_host(z[:-1], len(data))[1] == 1
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    z = co.compress(data) + co.flush()
    assert (z[2] >> 1) & 3 == 1 and P.inflate_host(z, len(data)) == (data, 0)
    assert P.inflate_host(b"", 4) == (b"", 1) and P.inflate_host(b"\x78", 4)[1] == 1 and P.inflate_host(b"\x78\x9c", 4)[1] == 1


def test_listing_rules(tmp_path):
    for n in ("10.png", "2.png", "2_seg.png", "10_seg.png", "3.png", "x.jpg", "7_seg.png"):
        Image.new("L", (4, 3)).save(tmp_path / n) if n.endswith(".png") else (tmp_path / n).write_bytes(b"")
    imgs, segs = P.bagls_pairs(str(tmp_path))
    assert [os.path.basename(p) for p in imgs] == ["10.png", "2.png"] and [os.path.basename(p) for p in segs] == ["10_seg.png", "2_seg.png"]
    assert [os.path.basename(p) for p in P.bagls_pairs(str(tmp_path), 1)[0]] == ["10.png"]
    assert P.bagls_pairs(str(tmp_path), 3)[0] == imgs                         # the cut comes before the pairs without a label leave
    assert len(P.png_files(str(tmp_path))) == 6
    with pytest.raises(OpenGlottalHipError, match="no .png"):
        os.makedirs(tmp_path / "empty")
        P.png_files(str(tmp_path / "empty"))
    b = io.BytesIO()
    Image.new("L", (4, 3), 9).save(b, "PNG")
    assert struct.unpack(">II", b.getvalue()[16:24]) == (4, 3) and P._ihdr_pixels(np.frombuffer(b.getvalue(), np.uint8)) == 12
