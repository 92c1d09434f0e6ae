"""`og_pnge_plan`: the launches of the streamed PNG encode walked without a device -- four per micro-batch, grids from the shape, a
workspace that does not grow with B, LDS of two segment workgroups within a CU's, and no launch writing past the caller's buffers."""
import pytest

from openglottal_amd import png as P
from openglottal_amd._lib import OpenGlottalHipError

LDS_PER_CU = 160 << 10
KERNELS = ["k_pnge_filter", "k_pnge_segment", "k_pnge_offsets", "k_pnge_place"]
SHAPES = ((1, 1, 1, 64), (5, 40, 3, 64), (64, 96, 3, 32768), (256, 256, 1, 32768), (256, 256, 3, 32768), (480, 640, 1, 256), (1080, 1920, 3, 32768),
          (4096, 4096, 3, 32768))


def writes(rec):
    return {} if rec["writes"] == "-" else {k: int(v) for k, v in (w.split("=") for w in rec["writes"].split(";"))}


def frame_ws(H, W, C, S):
    """the header's MEMORY paragraph"""
    N = H * (1 + W * C)
    nseg = -(-N // S)
    return ((N + 15) & ~15) + nseg * (S + 16 + 12) + 8 * H + 24, N, nseg


@pytest.mark.parametrize("H,W,C,S", SHAPES)
def test_launches_grids_lds_and_writes(H, W, C, S):
    per, N, nseg = frame_ws(H, W, C, S)
    bound = P.encode_bound(H, W, C, S)
    for B, chunk in ((1, 3), (3, 3), (7, 3), (130, 128)):
        recs, ws = P.encode_plan(B, H, W, C, S, chunk)
        assert [r["kernel"] for r in recs[:4]] == KERNELS and len(recs) % 4 == 0
        done = 0
        for i in range(0, len(recs), 4):
            f, s, o, p = recs[i:i + 4]
            assert [r["kernel"] for r in (f, s, o, p)] == KERNELS
            nb = s["gy"]
            assert nb == min(max(1, min(chunk, (256 << 20) // per)), B - done)
            assert (f["gx"], f["gy"], f["gz"], f["block"]) == ((nb * H + 3) // 4, 1, 1, 256)       # a wave per row
            assert (s["gx"], s["gz"], s["block"]) == (nseg, 1, 1024) and (p["gx"], p["gy"], p["block"]) == (nseg, nb, 256)
            assert (o["gx"], o["gy"], o["gz"], o["block"]) == (1, 1, 1, 1024) and nb <= 1024       # a thread per file
            for r in (f, s, o, p):
                assert 0 < r["gx"] < 2 ** 31 and r["gy"] <= 65535 and r["lds"] <= LDS_PER_CU
            assert s["lds"] == P.encode_limit(7) >= 2 * 32768 and 2 * s["lds"] <= LDS_PER_CU
            assert f["workspace"] >= nb * (per - 24) and f["workspace"] <= ws
            done += nb
            assert writes(f) == {} and writes(s) == {}                      # the workspace only
            assert writes(o) == {"sizes": 4 * done, "total": 8}
            assert writes(p) == {"out": done * bound}
        assert done == B
        assert max(writes(r).get("out", 0) for r in recs) == B * bound     # never past cap = B * bound
        assert max(writes(r).get("sizes", 0) for r in recs) == 4 * B


def test_micro_batches_at_chunk_3():
    for B, want in ((1, [1]), (3, [3]), (7, [3, 3, 1])):
        recs, _ = P.PngEncoder(chunk=3).plan(B, 64, 96, 3)
        assert [r["gy"] for r in recs if r["kernel"] == "k_pnge_segment"] == want
        assert [r["gx"] for r in recs if r["kernel"] == "k_pnge_filter"] == [(nb * 64 + 3) // 4 for nb in want]


@pytest.mark.parametrize("H,W,C", ((64, 64, 1), (256, 256, 3), (1080, 1920, 3)))
def test_the_workspace_does_not_grow_with_B(H, W, C):
    chunk = 16
    _, ws1 = P.encode_plan(chunk, H, W, C, 32768, chunk)
    for B in (chunk + 1, 4 * chunk, 1000):
        recs, ws = P.encode_plan(B, H, W, C, 32768, chunk)
        assert ws == ws1
        assert max(r["workspace"] for r in recs) <= ws
    _, small = P.encode_plan(2, H, W, C, 32768, chunk)
    assert small <= ws1


def test_bad_arguments():
    for args in ((0, 8, 8, 1, 64, 4), (1, 0, 8, 1, 64, 4), (1, 8, 8, 2, 64, 4), (1, 8, 8, 1, 64, 0), (1, 8, 8, 1, 64, 1025), (1, 4097, 4096, 1, 64, 4),
                 (1, 8, 8, 1, 100, 4), (1, 8, 8, 1, 65536, 4)):
        with pytest.raises(OpenGlottalHipError):
            P.encode_plan(*args)
