"""`og_mjpeg_plan`: the launches of the streamed JPEG pass walked without a device -- four per micro-batch, a workspace that does not
grow with B, LDS within a CU's, every interval's slot at least its worst case, and no launch writing past the caller's buffers."""
import pytest

from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import OpenGlottalHipError

LDS_PER_CU = 160 << 10
KERNELS = ["k_mjpeg_transform", "k_mjpeg_entropy", "k_mjpeg_offsets", "k_mjpeg_place"]
SHAPES = ((1, 1), (8, 8), (13, 21), (256, 256), (16, 720), (1080, 1920), (4096, 4096))


def writes(rec):
    return {} if rec["writes"] == "-" else {k: int(v) for k, v in (w.split("=") for w in rec["writes"].split(";"))}


def geometry(H, W):
    M = ((H + 7) // 8) * ((W + 7) // 8)
    return M, (M + MJ.limit(1) - 1) // MJ.limit(1)


@pytest.mark.parametrize("H,W", SHAPES)
def test_launches_grids_lds_and_writes(H, W):
    M, nI = geometry(H, W)
    bound = MJ.bound(H, W)
    for B, chunk in ((1, 128), (7, 3), (130, 128)):
        recs, ws = MJ.plan(B, H, W, chunk)
        assert [r["kernel"] for r in recs[:4]] == KERNELS and len(recs) % 4 == 0
        done = 0
        for i in range(0, len(recs), 4):
            t, e, o, p = recs[i:i + 4]
            nb = e["gy"]
            mb = max(1, min(chunk, (256 << 20) // (M * 384 + nI * (MJ.limit(5) + 12))))       # the header's MEMORY paragraph
            assert nb == min(mb, B - done)
            assert t["block"] == 256 and t["gx"] == (nb * M + 31) // 32 and (t["gy"], t["gz"]) == (1, 1)
            assert (e["gx"], e["block"]) == (nI, 64) and (p["gx"], p["gy"], p["block"]) == (nI, nb, 256)
            assert (o["gx"], o["gy"], o["gz"], o["block"]) == (1, 1, 1, 1024)
            for r in (t, e, o, p):
                assert 0 < r["gx"] < 2 ** 31 and r["gy"] <= 65535 and r["lds"] <= 64 << 10 <= LDS_PER_CU
            # the entropy kernel's LDS holds an interval's coefficients, its bit string and its stuffed bytes at their worst
            blocks = 3 * MJ.limit(1)
            assert e["lds"] >= blocks * 128 + blocks * 208 + MJ.limit(5)
            assert t["workspace"] >= nb * (M * 384 + nI * (MJ.limit(5) + 12))       # coefficients, slots, lengths, offsets
            done += nb
            assert writes(t) == {} and writes(e) == {}                      # the workspace only
            assert writes(o) == {"sizes": 4 * done, "total": 8}
            assert writes(p) == {"out": done * bound}
        assert done == B
        assert max(writes(r).get("out", 0) for r in recs) == B * bound     # never past cap = B * bound
        assert max(writes(r).get("sizes", 0) for r in recs) == 4 * B


def test_the_slot_is_the_worst_case_of_an_interval():
    ri = MJ.limit(1)
    bits = 63 * 26 + 22                                                     # every AC the longest code and 10 bits, the chroma DC 11 + 11
    stuffed = 2 * ((bits + 7) // 8)
    assert MJ.limit(5) >= 3 * ri * stuffed + 2
    assert MJ.bound(8, 8 * ri) == MJ.limit(6) + 3 * ri * stuffed + 2 + 2


@pytest.mark.parametrize("H,W", ((64, 64), (256, 256), (1080, 1920)))
def test_the_workspace_does_not_grow_with_B(H, W):
    chunk = 16
    _, ws1 = MJ.plan(chunk, H, W, chunk)
    for B in (chunk + 1, 4 * chunk, 1000):
        recs, ws = MJ.plan(B, H, W, chunk)
        assert ws == ws1
        assert max(r["workspace"] for r in recs) <= ws
    _, small = MJ.plan(2, H, W, chunk)
    assert small <= ws1


def test_bad_arguments():
    for args in ((0, 8, 8, 4), (1, 0, 8, 4), (1, 8, 8, 0), (1, 8, 8, 1025), (1, 4097, 4096, 4), (1, 8, 65536, 4)):
        with pytest.raises(OpenGlottalHipError):
            MJ.plan(*args)
