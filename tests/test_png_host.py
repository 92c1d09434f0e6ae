"""The host twin of the device PNG decoder (og_pngd_*_host, include_ext/openglottal_hip_png.h) against two other decoders: an
independent numpy unfilter over zlib.decompress (tests/png_cases.py) and Pillow.  Valid files: status 0 and the same bytes as both.
The hostile corpus: every status occurs, status 0 => Pillow's bytes, a non-zero status => every output byte 0.  The ring files and
the errors beyond the first window: each seam asserted from the file's tokens.  No GPU."""
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


def slot(p):
    return p & (PC.WINDOW - 1)


def wraps(p, n):
    """n bytes from p run past the end of the 32 KiB ring"""
    return slot(p) + n > PC.WINDOW


@pytest.mark.parametrize("name", list(PC.ring_files()))
def test_the_ring_files_hold_what_they_claim(name):
    """the firing checks: every seam a ring file is named for, computed from its tokens.  A file that stops reaching its seam fails
    here instead of going quiet."""
    r = PC.ring_files()[name]
    toks, stride = r.tokens, 1 + r.W
    m, w, spans = PC.match_facts(toks), PC.writers(toks), PC.token_spans(toks)
    info = P.parse(r.file)
    assert (info["ctype"], info["depth"], info["raw_bytes"]) == (0, 8, len(r.raw)) and len(r.raw) <= 131042
    assert PC.lz_expand(toks) == r.raw == zlib.decompress(r.z) and all(r.raw[y * stride] <= 4 for y in range(r.H))
    is_stored = lambda i: not isinstance(toks[i], int) and toks[i][0] == "S"   # noqa: E731
    src = lambda p, n, d: range(p - d, p - d + min(n, d))   # noqa: E731
    if name == "ring-stored-match":                                           # R1
        (p0, n0, d0), (p1, n1, d1) = m
        assert p0 + n0 <= PC.WINDOW and {w[q] for q in src(p0, n0, d0)} == {0} and is_stored(0)
        by, = {w[q] for q in src(p1, n1, d1)}
        assert is_stored(by) and wraps(*spans[by]) and p1 - spans[by][0] - spans[by][1] == 0 and p1 < 2 * PC.WINDOW
        assert p1 - d1 < PC.WINDOW < p1 - d1 + n1                             # the source spans the wrap point the stored block crossed
    elif name in ("ring-wrap-258", "ring-wrap-3"):                            # R2, R3
        n = 258 if name == "ring-wrap-258" else 3
        across = [(p, ln, d) for p, ln, d in m if wraps(p, ln) and ln == n]
        assert sorted(d > ln for _, ln, d in across) == [False, True] and len({p >> 15 for p, _, _ in across}) == 2
        assert n != 3 or all(slot(p) == PC.WINDOW - 2 for p, _, _ in across)  # two bytes before the wrap, one behind it
        assert any(wraps(p - d, min(ln, d)) and (d > ln) == (n == 258) for p, ln, d in m)
    elif name == "ring-self-overwrite":                                       # R4
        own = {(PC.WINDOW - d, min(p >> 15, 2)) for p, ln, d in m if ln == 258 and d + ln > PC.WINDOW}
        assert own == {(k, 1) for k in PC.R4_GAPS} | {(k, 2) for k in (0,) + PC.R4_GAPS} and (66078, 258, PC.WINDOW) in m
        assert {1, 63} <= set(PC.R4_GAPS) and {64, 65, 100, 257} <= set(PC.R4_GAPS)   # the same turn, the next turn's same lane, later turns
    elif name == "ring-short-dist":                                           # R5, R6
        assert {(ln, d) for p, ln, d in m if p + ln <= PC.WINDOW} >= {(258, d) for d in (1, 2, 3, 63, 64, 65, 127, 128, 129, 257)} | {(64, 1), (65, 1)}
        at_once = [spans[i][0] for i in range(1, len(toks)) if isinstance(toks[i - 1], int) and not isinstance(toks[i], int) and toks[i][1] == 1]
        assert any(slot(p) == 0 and p for p in at_once) and any(0 < p < PC.WINDOW for p in at_once)
    elif name == "ring-tables":                                               # R7
        assert [b[0] for b in r.blocks] == ["dynamic", "dynamic", "fixed", "stored", "dynamic"] and (r.z[2] >> 1) & 3 == 2
        (l0, d0), (l1, d1), (l4, d4) = (PC.token_syms(r.blocks[i][1]) for i in (0, 1, 4))
        assert max(l0) + 1 == 286 and max(l1) + 1 == 258 and len(set(l1)) < len(set(l0)) // 4    # HLIT; lsym keeps the old symbols behind the new
        assert max(d0) + 1 > 20 and len(set(d0)) > 5 and set(d1) == {0} and len(set(d4)) > 2      # HDIST 1, one distance code
        assert all(r.marks[i][0] % 8 for i in (1, 2, 3))                      # headers off the byte grid
    else:                                                                     # R8
        assert len(r.raw) in (65521, 131042) and len(r.raw) % 65521 == 0 and all(b[0] == "stored" for b in r.blocks)
        assert set(r.raw[1:stride]) == {255} and set(r.raw[-r.W:]) == {255} and r.raw.count(255) == r.H * r.W


def test_the_other_new_files_hold_what_they_claim():
    files = dict(VALID)
    for n, depth in (("wide-gray-1", 1), ("wide-pal-2", 2), ("wide-gray-4", 4)):
        i = P.parse(files[n])
        assert i["depth"] == depth and i["W"] > 1000 and (i["W"] * depth) % 8 and i["rb"] == (i["W"] * depth + 7) // 8
    i = P.parse(files["paeth-rgba-65x600"])
    assert (i["H"], i["rb"], i["bpp"]) == (65, 2400, 4) and set(zlib.decompress(PC.stream_of(files["paeth-rgba-65x600"]))[::2401]) == {4}
    i = P.parse(files["average-paeth-1000x3"])
    assert (i["H"], i["W"], (i["H"] + 63) // 64) == (1000, 3, 16) and zlib.decompress(PC.stream_of(files["average-paeth-1000x3"]))[:12:4] == bytes([3, 4, 3])
    assert [n for n, _ in VALID[:75]][-1] == "far-match-32768" and len(VALID) == 75 + len(PC.ring_files()) + 5


def test_errors_beyond_the_first_window():
    """every deep-error file meets its error where its name says (from the tokens), gives its status and zeros; zlib refuses it,
    or accepts it with another size (4) or with a row start of 5 (7)"""
    cases = {n: (f, s, pos) for n, f, s, pos in PC.deep_errors()}
    assert sorted(s for _, s, _ in cases.values()) == [1, 1, 2, 2, 3, 4, 4, 4, 5, 7]
    for name, (f, want, pos) in cases.items():
        px, st = P.decode_host(f, 3, statuses=True)
        assert st == want and px is not None and not px.any() and not P.decode_host(f, 1, statuses=True)[0].any(), (name, st)
        cap, z = P.parse(f)["raw_bytes"], PC.stream_of(f)
        if want in (4, 7):
            raw = zlib.decompress(z)
            assert (len(raw) > cap) if want == 4 else (len(raw) == cap and raw[pos] == 5), name
        else:
            with pytest.raises(zlib.error):
                zlib.decompress(z)
        assert P.inflate_host(z, cap)[1] == (0 if want == 7 else want), name
    at = {n: pos for n, (_, _, pos) in cases.items()}
    cap = lambda n: P.parse(cases[n][0])["raw_bytes"]   # noqa: E731
    assert PC.WINDOW < at["deep-cut-in-stored"] and 2 * PC.WINDOW <= at["deep-cut-in-distance-extra"] and PC.WINDOW < at["deep-litlen-286"]
    tables = PC.ring_files()["ring-tables"]
    assert at["deep-third-header-over-subscribed"] == tables.block_pos(4) and [b[0] for b in tables.blocks[:5]].count("dynamic") == 3
    for n, length in (("deep-overflow-literal", 1), ("deep-overflow-match", 258), ("deep-overflow-stored", 501)):
        assert cap(n) > 65536 and at[n] + length == cap(n) + 1 and at[n] >> 15 == cap(n) >> 15 == 2, n
    assert at["deep-adler-flip"] > 65521 and at["deep-adler-flip"] % 250 and cap("deep-adler-flip") == 272 * 250
    assert at["deep-filter-5-by-match"] % 100 == 0 and at["deep-filter-5-by-match"] // 100 >= 64


def test_distance_32768_is_refused_at_32767_and_taken_at_32768():
    bad = {n: f for n, f, _, _ in PC.deep_errors()}["distance-32768-at-32767"]
    good = dict(VALID)["far-match-32768"]
    assert P.decode_host(bad, statuses=True)[1] == 3 and P.decode_host(good, statuses=True)[1] == 0
    assert P.parse(bad)["raw_bytes"] == P.parse(good)["raw_bytes"]
    # the valid file's stream: 32 768 literals of the fixed code, then length 258 at distance 32 768; the refused one: one byte fewer
    raw = zlib.decompress(PC.stream_of(good))
    assert raw[32768:32768 + 258] == raw[:258] and raw[32768 + 258] != raw[258]


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
