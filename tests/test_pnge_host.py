"""The host twin of the device PNG encoder (include_enc/openglottal_hip_pnge.h; `png.encode_host`, `png.filter_host`,
`png.deflate_host`) on the case list of tests/pnge_cases.py.  The judges are independent of the code under test: Pillow and this
project's decoder for the pixels, zlib for the stream, a numpy filter for the raw bytes, the numpy unfilter of tests/png_cases.py, and
a plain Python inflate (`pnge_cases.blocks`) that shows every block's header and tokens.  No GPU."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

import pnge_cases as EC
import png_cases as PC
from openglottal_amd import png as P

# largest twin / zlib ratio measured on COMPRESSION_SET (1.1331, a letterboxed mask tile of 315 bytes against 278),
# rounded up to the next whole percent; the images alone stay below 1.006
RATIO_GATE = 1.14
IMAGE_RATIO_GATE = 1.01


def zlib_rle(raw):
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_RLE)
    return c.compress(raw) + c.flush()


def expected_tokens(seg):
    """the tokens of one segment by the rule of the header: [(length or 0, literal or None)]"""
    out = []
    lengths, values = EC.run_lengths(seg)
    for n, v in zip(lengths.tolist(), values.tolist()):
        out.append((0, v))
        R = n - 1
        out += [(258, None)] * (R // 258)
        r = R % 258
        out += [(r, None)] if r >= 3 else [(0, v)] * r
    return out


def segment_blocks(z):
    """the blocks of a stream without the empty stored blocks that close a dynamic segment off the byte grid; those are checked here"""
    out = []
    for b in EC.blocks(z):
        if b["type"] == 0 and b["n"] == 0 and not b["final"]:
            assert out and out[-1]["type"] == 2 and out[-1]["end"] % 8 != 0 and b["start"] == out[-1]["end"]
            assert b["end"] % 8 == 0 and z[2 + b["end"] // 8 - 4:2 + b["end"] // 8] == b"\x00\x00\xff\xff"
            assert b["end"] - b["start"] <= 3 + 7 + 32
            continue
        assert b["start"] % 8 == 0, "every segment starts on a byte"
        out.append(b)
    return out


@pytest.mark.parametrize("cid", [c[0] for c in EC.cases()])
def test_round_trip(cid):
    _, f, S = EC.by_id(cid)
    H, W, C = f.shape
    png = P.encode_host(f, S)
    assert len(png) <= P.encode_bound(H, W, C, S)
    im = Image.open(io.BytesIO(png))
    assert im.mode == ("L" if C == 1 else "RGB") and np.array_equal(np.asarray(im), f[..., 0] if C == 1 else f[..., ::-1])
    out, st = P.decode_host(png, C, statuses=True)
    assert st == 0 and np.array_equal(out, f)
    raw = P.filter_host(f)
    z = EC.idat(png)                                                          # (one IDAT; every chunk's CRC is checked there)
    assert z[:2] == b"\x78\x01" and zlib.decompress(z) == raw and P.deflate_host(raw, S) == z
    assert raw == EC.raw_reference(f)
    assert np.array_equal(PC.reference(png, C), f)
    info = P.parse(png)
    assert (info["H"], info["W"], info["ctype"], info["depth"], info["nidat"], info["status"]) == (H, W, 0 if C == 1 else 2, 8, 1, 0)


@pytest.mark.parametrize("cid", ["runs-c1-s64", "runs-c1-s256", "runs-c1-s32768", "zeros-4x50-c1-s64", "seam-rows-c1-s64", "all-literals-c1-s256",
                                 "filters-c3-s64", "raw-S+1-64-c1-s64", "raw-2S-256-c1-s256", "two-segments-181x182-c1-s32768"])
def test_segments_and_tokens(cid):
    """Every segment is one block that gives exactly its S bytes (the last one the rest), its tokens are those of the rule applied to
    the segment alone -- so a run that crosses a seam is cut there -- and its code sets are complete."""
    _, f, S = EC.by_id(cid)
    raw = P.filter_host(f)
    bl = segment_blocks(P.deflate_host(raw, S))
    assert [b["n"] for b in bl] == [min(S, len(raw) - o) for o in range(0, len(raw), S)]
    assert [b["final"] for b in bl] == [0] * (len(bl) - 1) + [1]
    for k, b in enumerate(bl):
        seg = raw[k * S:(k + 1) * S]
        if b["type"] == 0:
            assert b["data"] == seg
            continue
        assert b["tokens"] == expected_tokens(seg), (cid, k)
        assert EC.kraft(b["lit_lens"]) == 1.0 and max(b["lit_lens"]) <= 15 and b["dist_lens"] == [1] and EC.kraft(b["cl_lens"]) == 1.0
        assert max(b["cl_lens"]) <= 7 and (len(b["lit_lens"]) == 257 or b["lit_lens"][-1] > 0)
        assert (b["end"] - b["start"] + 7) // 8 < 5 + len(seg), "a dynamic block is only taken when it is smaller than the stored one"


def test_the_runs_case_holds_every_run_length():
    _, f, _ = EC.by_id("runs-c1-s32768")
    raw = P.filter_host(f)
    d = EC.runs_bytes(EC.RUNS + (32768,))
    assert raw == bytes([1] + d)                                              # Sub gives the string the row was summed from
    lengths, values = EC.run_lengths(raw)
    assert set(EC.RUNS) | {32768} <= set(lengths[values == 0].tolist())
    toks = [t for b in segment_blocks(P.deflate_host(raw, 32768)) for t in b["tokens"]]
    assert toks == expected_tokens(raw[:32768]) + expected_tokens(raw[32768:])
    assert {n for n, _ in toks} >= {0, 3, 257, 258}                          # a run of 4 is a literal and a match of 3, one of 258 a match of 257
    # a run across the seam at S = 64: the zero run of 258 starts inside one segment and ends three segments on
    cut = segment_blocks(P.deflate_host(raw, 64))
    assert all(n <= 63 for b in cut for n, _ in b["tokens"])
    # a segment of one distinct byte: a literal and one match of S - 1
    one = [b for b in cut if b["type"] == 2 and b["tokens"] == [(0, 0), (63, None)]]
    assert one and sum(1 for l in one[0]["lit_lens"] if l) == 3


def test_each_filter_wins_a_row_and_ties_go_to_the_lower_type():
    _, f, _ = EC.by_id("filters-c1-s32768")
    cost, _ = EC.filter_costs(f)
    raw = np.frombuffer(P.filter_host(f), np.uint8).reshape(f.shape[0], -1)
    chosen = raw[:, 0]
    assert chosen.tolist() == cost.argmin(1).tolist() and set(chosen.tolist()) == {0, 1, 2, 3, 4}
    ties = [r for r in range(f.shape[0]) if (cost[r] == cost[r].min()).sum() > 1]
    assert ties and all(chosen[r] == int(np.flatnonzero(cost[r] == cost[r].min())[0]) for r in ties)
    assert (cost[-1] == 0).all() and chosen[-1] == 0                          # the zero row under a zero row: all five tie
    for cid in ("filters-c3-s64", "two-segments-181x182-c3-s32768", "synth0-c3-s32768"):
        g = EC.by_id(cid)[1]
        c3, _ = EC.filter_costs(g)
        assert np.frombuffer(P.filter_host(g), np.uint8).reshape(g.shape[0], -1)[:, 0].tolist() == c3.argmin(1).tolist(), cid


def test_a_zero_frame_is_three_small_segments():
    f = EC.by_id("zeros-256-c1-s32768")[1]
    png = P.encode_host(f)
    bl = segment_blocks(EC.idat(png))
    assert [b["n"] for b in bl] == [32768, 32768, 256 * 257 - 65536] and all(b["type"] == 2 for b in bl)
    assert [len(b["tokens"]) for b in bl] == [129, 129, 2]                    # 32 768 = a literal, 127 matches of 258, a literal
    assert bl[0]["tokens"] == expected_tokens(bytes(32768)) and bl[2]["tokens"] == [(0, 0), (255, None)]
    assert len(png) < 3 * 200 + 100 and len(png) <= P.encode_bound(256, 256, 1)
    assert P.encode_bound(256, 256, 1) == 57 + 2 + 4 + 256 * 257 + 5 * 3
    assert P.encode_bound(5, 40, 3, 64) == 57 + 6 + 5 * 121 + 5 * 10 and P.encode_limit(6) == 57


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("S", EC.SEGMENTS)
def test_noise_is_stored_and_does_not_grow(C, S):
    f = EC.by_id(f"noise-c{C}-s{S}")[1]
    png = P.encode_host(f, S)
    raw = P.filter_host(f)
    bl = EC.blocks(EC.idat(png))
    nseg = -(-len(raw) // S)
    assert len(bl) == nseg and all(b["type"] == 0 for b in bl)
    assert len(png) == P.encode_bound(f.shape[0], f.shape[1], C, S) <= len(raw) + 10 * nseg + 57 + 6


def test_fibonacci_counts_are_limited_to_fifteen_bits():
    _, f, S = EC.by_id("fibonacci-c1-s32768")
    raw = P.filter_host(f)
    assert raw == bytes([1] + EC.fibonacci_bytes()) and len(raw) <= S
    freq = np.bincount(np.frombuffer(raw, np.uint8), minlength=257)
    freq[256] = 1
    assert EC.huffman_depth(freq.tolist()) > 15                               # an unlimited code would not fit
    b, = segment_blocks(P.deflate_host(raw, S))
    assert b["type"] == 2 and max(b["lit_lens"]) == 15 and EC.kraft(b["lit_lens"]) == 1.0
    assert sorted(s for s, l in enumerate(b["lit_lens"]) if l) == sorted(set(raw) | {256})
    order = sorted((s for s in set(raw)), key=lambda s: -freq[s])             # a more frequent byte never has the longer code
    assert all(b["lit_lens"][a] <= b["lit_lens"][c] for a, c in zip(order, order[1:]))


def test_all_literals_and_several_length_codes():
    _, f, S = EC.by_id("all-literals-c1-s32768")
    raw = P.filter_host(f)
    assert raw == bytes([1] + EC.all_literals_bytes())
    b, = segment_blocks(P.deflate_host(raw, S))
    used = {s for s, l in enumerate(b["lit_lens"]) if l}
    assert set(range(257)) <= used and len(used - set(range(257))) >= 3


def test_the_default_segment_gives_two_real_segments_on_181x182():
    f = EC.by_id("two-segments-181x182-c1-s32768")[1]
    raw = P.filter_host(f)
    assert len(raw) == 33124
    assert [(b["type"], b["n"]) for b in segment_blocks(EC.idat(P.encode_host(f)))] == [(2, 32768), (2, 356)]


def test_compression_against_zlib_rle():
    """zlib level 6 with Z_RLE over the twin's own filtered bytes is the yardstick; both sides are deterministic integer programs."""
    fr, gt = EC.synth_frames()
    ti, tm = EC.crop_tiles()
    worst, worst_image = 0.0, 0.0
    for name, arr, image in (("frame", fr, True), ("mask", gt, False), ("tile", ti, True), ("tile-mask", tm, False)):
        for i, f in enumerate(arr):
            raw = P.filter_host(f)
            mine, ref = len(P.deflate_host(raw)), len(zlib_rle(raw))
            b = io.BytesIO()
            Image.fromarray(f).save(b, "PNG")
            print(f"{name}{i}: twin {mine} zlib Z_RLE {ref} ratio {mine / ref:.4f}; file {len(P.encode_host(f))} Pillow {len(b.getvalue())}")
            worst = max(worst, mine / ref)
            if image:
                worst_image = max(worst_image, mine / ref)
    assert worst <= RATIO_GATE and worst_image <= IMAGE_RATIO_GATE, (worst, worst_image)


def test_the_python_twin_refuses_what_the_header_leaves_out():
    with pytest.raises(P.OpenGlottalHipError):
        P.encode_host(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(P.OpenGlottalHipError):
        P.encode_host(np.zeros((4, 4), np.uint8), segment=96)
    with pytest.raises(P.OpenGlottalHipError):
        P.encode_host(np.zeros((4, 4), np.uint8), segment=65536)
    with pytest.raises(P.OpenGlottalHipError):
        P.encode_bound(4097, 4096, 1)
    assert P.encode_host(np.zeros((4, 4), np.uint8)) == P.encode_host(np.zeros((4, 4, 1), np.uint8))
