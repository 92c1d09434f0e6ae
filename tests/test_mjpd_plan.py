"""`og_mjpd_plan`: the launches of the streamed JPEG decode walked without a device -- four per micro-batch and no others, a workspace
that does not grow with B, LDS within a CU's, a lane per restart interval, and no launch writing past the caller's buffers."""
import pytest

from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import OpenGlottalHipError

LDS_PER_CU = 160 << 10
KERNELS = ["k_mjpd_markers", "k_mjpd_entropy", "k_mjpd_idct", "k_mjpd_colour"]
SHAPES = ((1, 1), (8, 8), (17, 9), (37, 50), (256, 256), (480, 640), (1080, 1920), (4096, 4096))


def writes(rec):
    return {} if rec["writes"] == "-" else {k: int(v) for k, v in (w.split("=") for w in rec["writes"].split(";"))}


def geometry(H, W, sampling):
    """`(M, blocks per frame)` from the header's FORMAT paragraph."""
    hl, vl = (2 if sampling >= 2 else 1), (2 if sampling == 3 else 1)
    mx, my = -(-W // (8 * hl)), -(-H // (8 * vl))
    return mx * my, mx * my * (hl * vl + (2 if sampling else 0))


@pytest.mark.parametrize("sampling", (0, 1, 2, 3))
@pytest.mark.parametrize("H,W", SHAPES)
def test_launches_grids_lds_and_writes(H, W, sampling):
    M, blocks = geometry(H, W, sampling)
    for Ri in (0, 1, 16):
        nI = -(-M // Ri) if Ri else 1
        per_frame = blocks * 192 + nI * 8 + 4                              # the header's MEMORY paragraph
        for B, chunk in ((1, 128), (7, 3), (130, 128)):
            recs, ws = MJ.decode_plan(B, H, W, sampling, Ri, chunk)
            assert [r["kernel"] for r in recs] == KERNELS * (len(recs) // 4)      # closed against the four kernels
            mb = max(1, min(chunk, (256 << 20) // per_frame))
            done = 0
            for i in range(0, len(recs), 4):
                m, e, t, c = recs[i:i + 4]
                nb = m["gx"]
                assert nb == min(mb, B - done)
                assert (m["gy"], m["gz"], m["block"]) == (1, 1, 256)
                assert (e["gx"], e["gy"], e["gz"], e["block"]) == (-(-nb * nI // 64), 1, 1, 64)      # a lane per interval
                assert (t["gx"], t["gy"], t["gz"], t["block"]) == (-(-nb * blocks // 32), 1, 1, 256)   # 8 lanes per block
                assert (c["gx"], c["gy"], c["gz"], c["block"]) == (-(-H * W // 256), nb, 1, 256)       # a lane per pixel
                for r in (m, e, t, c):
                    assert 0 < r["gx"] < 2 ** 31 and r["gy"] <= 65535 and r["lds"] <= 64 << 10 <= LDS_PER_CU
                assert e["lds"] == MJ.decode_limit(3) and t["lds"] == 32 * 8 * 9 * 4 and m["lds"] == c["lds"] == 0
                assert m["workspace"] == nb * per_frame <= max(256 << 20, per_frame)
                done += nb
                assert writes(m) == {"status": 4 * done} and writes(e) == {"status": 4 * done}
                assert writes(t) == {}                                      # the workspace only
                assert writes(c) == {"frames": done * H * W * 3}
            assert done == B
            assert max(writes(r).get("frames", 0) for r in recs) == B * H * W * 3      # never past cap = B * H * W * 3
            assert max(writes(r).get("status", 0) for r in recs) == 4 * B


@pytest.mark.parametrize("H,W", ((64, 64), (256, 256), (480, 640)))
def test_the_workspace_does_not_grow_with_B(H, W):
    chunk = 16
    _, ws1 = MJ.decode_plan(chunk, H, W, 3, 0, chunk)
    for B in (chunk + 1, 4 * chunk, 1000):
        recs, ws = MJ.decode_plan(B, H, W, 3, 0, chunk)
        assert ws == ws1
        assert max(r["workspace"] for r in recs) <= ws
    _, small = MJ.decode_plan(2, H, W, 3, 0, chunk)
    assert small <= ws1
    assert MJ.MjpegDecoder(chunk=chunk).plan(chunk, H, W, 3, 0) == MJ.decode_plan(chunk, H, W, 3, 0, chunk)


def test_bad_arguments():
    for args in ((0, 8, 8, 1, 0, 4), (1, 0, 8, 1, 0, 4), (1, 8, 8, 1, 0, 0), (1, 8, 8, 1, 0, 1025), (1, 4097, 4096, 1, 0, 4), (1, 8, 65536, 1, 0, 4),
                 (1, 8, 8, 4, 0, 4), (1, 8, 8, -1, 0, 4), (1, 8, 8, 1, -1, 4), (1, 8, 8, 1, 65536, 4)):
        with pytest.raises(OpenGlottalHipError):
            MJ.decode_plan(*args)
