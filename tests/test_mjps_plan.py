"""`og_mjps_plan`: with the mode off, or with restart markers, `og_mjpd_plan`'s text; with the mode on and Ri == 0 four launches per
micro-batch and no others -- k_mjps_entropy a workgroup of 256 per frame in place of the lane per interval -- LDS within 64 KiB, no
launch writing past the caller's buffers, and a workspace that does not grow with B.  No device."""
import ctypes as C

import pytest

from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import OpenGlottalHipError, lib
from test_mjpd_plan import SHAPES, geometry, writes

KERNELS = ["k_mjpd_markers", "k_mjps_entropy", "k_mjpd_idct", "k_mjpd_colour"]


def text(fn, *args):
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong()
    n = fn(*args, out, len(out), C.byref(ws))
    return n, out.value, ws.value


@pytest.mark.parametrize("H,W", ((17, 9), (480, 640)))
def test_mode_0_and_files_with_markers_give_og_mjpd_plan_s_text(H, W):
    l = lib()
    for sampling in (0, 3):
        for Ri in (0, 1, 16):
            want = text(l.og_mjpd_plan, 7, H, W, sampling, Ri, 3)
            assert want[0] > 0
            for mode, sub in ((0, 0), (0, 64)) + (((1, 0), (1, 4)) if Ri else ()):
                assert text(l.og_mjps_plan, 7, H, W, sampling, Ri, 3, mode, sub) == want
            assert MJ.decode_plan(7, H, W, sampling, Ri, 3, "off") == MJ.decode_plan(7, H, W, sampling, Ri, 3)
    assert MJ.MjpegDecoder(chunk=3).plan(7, H, W, 3, 0) == MJ.decode_plan(7, H, W, 3, 0, 3)


@pytest.mark.parametrize("sampling", (0, 1, 2, 3))
@pytest.mark.parametrize("H,W", SHAPES)
def test_mode_1_launches_grids_lds_and_writes(H, W, sampling):
    M, blocks = geometry(H, W, sampling)
    per_frame = blocks * 192 + 8 + 4                                           # the tenth header's MEMORY paragraph: no new workspace
    for sub in (0, 4, 64, 1024):
        for B, chunk in ((1, 128), (7, 3), (130, 128)):
            recs, ws = MJ.decode_plan(B, H, W, sampling, 0, chunk, "auto", sub)
            assert [r["kernel"] for r in recs] == KERNELS * (len(recs) // 4)      # closed against the four kernels
            old, ws_old = MJ.decode_plan(B, H, W, sampling, 0, chunk)
            assert ws == ws_old and len(old) == len(recs)
            mb = max(1, min(chunk, (256 << 20) // per_frame))
            done = 0
            for i in range(0, len(recs), 4):
                m, e, t, c = recs[i:i + 4]
                nb = m["gx"]
                assert nb == min(mb, B - done)
                assert (e["gx"], e["gy"], e["gz"], e["block"]) == (nb, 1, 1, 256)      # a workgroup per frame
                assert e["lds"] == MJ.split_limit(5) <= 64 << 10 and e["workspace"] == 0
                assert [m, t, c] == [old[i], old[i + 2], old[i + 3]]                   # the other three launches are the old ones
                done += nb
                assert writes(e) == {"status": 4 * done} and writes(c) == {"frames": done * H * W * 3}
            assert done == B
            assert max(writes(r).get("frames", 0) for r in recs) == B * H * W * 3
            assert max(writes(r).get("status", 0) for r in recs) == 4 * B


@pytest.mark.parametrize("H,W", ((64, 64), (480, 640)))
def test_the_workspace_does_not_grow_with_B(H, W):
    chunk = 16
    _, ws1 = MJ.decode_plan(chunk, H, W, 3, 0, chunk, "auto")
    for B in (chunk + 1, 4 * chunk, 1000):
        recs, ws = MJ.decode_plan(B, H, W, 3, 0, chunk, "auto")
        assert ws == ws1 and max(r["workspace"] for r in recs) <= ws
    d = MJ.MjpegDecoder(chunk=chunk, split="auto", sub=32)
    assert d.plan(chunk, H, W, 3, 0) == MJ.decode_plan(chunk, H, W, 3, 0, chunk, "auto", 32)
    assert [r["kernel"] for r in d.plan(chunk, H, W, 3, 0)[0]] == KERNELS


def test_bad_arguments():
    for args in ((1, 8, 8, 1, 0, 4, "auto", 6), (1, 8, 8, 1, 0, 4, "auto", 2048), (1, 8, 8, 1, 0, 4, "on", 0), (0, 8, 8, 1, 0, 4, "auto", 0),
                 (1, 8, 8, 4, 0, 4, "auto", 0), (1, 8, 8, 1, 0, 0, "auto", 0)):
        with pytest.raises(OpenGlottalHipError):
            MJ.decode_plan(*args)
    assert lib().og_mjps_plan(1, 8, 8, 1, 0, 4, 2, 0, C.create_string_buffer(64), 64, None) == -1
