"""og_classic_plan: the launches, grids and workspace of the streamed guided-VFT pass per micro-batch, walked without a GPU:
one workgroup per frame for the blob filter, the micro-batch rule min(chunk, 64 MiB / (H * W * channels)), every write inside the
micro-batch's buffers, and device memory independent of the number of frames."""
import ctypes as C

import pytest

from openglottal_amd import classic as CL
from openglottal_amd._lib import OpenGlottalHipError, lib

MiB = 1 << 20


def micro_batch(chunk, H, W, ch):
    return max(1, min(chunk, (64 * MiB) // (H * W * ch)))


@pytest.mark.parametrize("B,H,W,ch,chunk", [(1, 64, 64, 1, 32), (70, 32, 48, 3, 32), (70, 256, 256, 3, 32), (2000, 256, 256, 3, 64),
                                            (5, 17, 23, 1, 2), (9, 120, 160, 3, 32), (3, 256, 256, 1, 128), (1500, 256, 256, 3, 1024)])
def test_plan_walks_the_micro_batches(B, H, W, ch, chunk):
    recs, ws = CL.plan(B, H, W, ch, chunk)
    mb = micro_batch(chunk, H, W, ch)
    n_batches = -(-B // mb)
    assert len(recs) == 3 * n_batches
    gz_limit = lib().og_workspace_limit(2)
    left = B
    for k in range(n_batches):
        nb = min(mb, left)
        left -= nb
        hist, thr, blobs = recs[3 * k:3 * k + 3]
        assert hist["kernel"].startswith("k_box_hist<") and (hist["gx"], hist["gy"], hist["gz"], hist["block"]) == (4, nb, 1, 256)
        assert thr["kernel"] == "k_vft_thresholds" and (thr["gx"], thr["gy"], thr["gz"], thr["block"]) == (1, 1, 1, 256)   # ONE workgroup walks the frames in order
        assert blobs["kernel"] == f"k_blobs<{ch}>" and (blobs["gx"], blobs["gy"], blobs["gz"], blobs["block"]) == (nb, 1, 1, 1024)   # one workgroup per frame
        assert blobs["workspace"] == nb * H * W * 8                                                      # two int32 label arrays per frame
        assert blobs["writes"] == f"mask={nb * H * W};area={4 * nb}"                                        # inside the micro-batch's buffers
        for r in (hist, thr, blobs):
            assert r["lds"] == 0 and max(r["gy"], r["gz"]) <= gz_limit and r["gx"] < 1 << 31 and r["counters"] == 0   # (lds: dynamic only)
    assert left == 0
    cb = min(mb, B)
    assert ws == cb * (H * W * (ch + 1 + 8) + 1060) + 8
    assert cb * H * W * ch <= max(64 * MiB, H * W * ch)


def test_device_memory_does_not_depend_on_the_number_of_frames():
    sizes = {CL.plan(B, 256, 256, 3, 32)[1] for B in (32, 33, 1000, 100000)}
    assert len(sizes) == 1 and sizes.pop() == 32 * (65536 * 12 + 1060) + 8
    assert CL.plan(5, 256, 256, 3, 32)[1] < CL.plan(32, 256, 256, 3, 32)[1]


def test_plan_refuses_what_the_entries_refuse():
    limit = lib().og_classic_limit(0)
    for args in ((0, 8, 8, 1, 32), (1, 0, 8, 1, 32), (1, 8, 8, 2, 32), (1, 8, 8, 1, 0), (1, 8, 8, 1, 1025), (1, 256, 257, 1, 32)):
        with pytest.raises(OpenGlottalHipError):
            CL.plan(*args)
    assert str(limit) in lib().og_last_error().decode()
    out = C.create_string_buffer(8)
    assert lib().og_classic_plan(70, 32, 48, 1, 32, out, 8, None) == -1 and b"does not fit" in lib().og_last_error()
    assert limit == 65536 and CL.plan(1, 256, 256, 1, 32)[1] == 65536 * 10 + 1060 + 8          # the largest frame
    assert len(CL.plan(1500, 256, 256, 3, 1024)[0]) == 3 * 5                                 # 64 MiB / 196 608 = 341 frames bind below chunk 1024
