"""-m gpu: the device-touching entry points of include/openglottal_hip_mjpeg.h held to the buffer extents their callers declare
(tests/buffer_guard.py): guards untouched, nothing written at or past out[total], sizes and total written whole, results independent
of the slack around the frames, the frames unchanged -- and the bytes equal to the host twin's.  `out` is declared at its capacity
and filled only up to `total`, so the three-run comparison of `run_guarded` (every declared byte written) does not apply; the single
guarded runs do."""
import numpy as np
import pytest

import buffer_guard as G
import mjpeg_cases as MC
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

OG_EINVAL = -1
CASES = ("batch7", "13x21-noise-q100", "wide-overlay", "wrap-steps-q100")

# entry point -> the test of this module that puts it inside guards
MJPEG_MATRIX = {
    "og_mjpeg_encode_u8_dev": "test_resident_frames",
    "og_mjpeg_encode_stream_u8": "test_host_streaming",
}


def held(entry, kind, cid, sync=None):
    c = MC.BY_ID[cid]
    B, H, W = c.frames.shape[:3]
    files = MC.host_files(cid)
    want = np.frombuffer(b"".join(files), np.uint8)
    cap = B * MJ.bound(H, W)
    e = MJ.Mjpeg(quality=c.quality, chunk=3)
    for slack in (0x00, 0xFF):
        rc, pay, faults = G.guarded_call(lambda p: entry(e._h, p["frames"], B, H, W, p["out"], cap, p["sizes"], p["total"]),
                                         {"frames": c.frames}, {"out": cap, "sizes": 4 * B, "total": 8}, kind,
                                         sync=(lambda: check(lib().og_mjpeg_sync(e._h), "og_mjpeg_sync")) if sync else None, slack=slack)
        assert rc == 0 and not faults, (cid, slack, faults)
        total = int(pay["total"].view(np.int64)[0])
        assert total == want.size and pay["sizes"].view(np.int32).tolist() == [len(j) for j in files], cid
        assert np.array_equal(pay["out"][:total], want), cid
        assert (pay["out"][total:] == G.GUARD_FILL).all(), (cid, "written past total")
        G.CASES[entry.__name__] += 1


@pytest.mark.parametrize("cid", CASES)
def test_host_streaming(cid):
    held(lib().og_mjpeg_encode_stream_u8, "host", cid)


@pytest.mark.parametrize("cid", CASES)
def test_resident_frames(cid):
    held(lib().og_mjpeg_encode_u8_dev, "device", cid, sync=True)


def test_refusals_leave_all_guards_intact_and_the_handle_usable():
    c = MC.BY_ID["batch7"]
    B, H, W = c.frames.shape[:3]
    cap = B * MJ.bound(H, W)
    e = MJ.Mjpeg(chunk=3)
    calls = {
        "sizes+1": lambda p: lib().og_mjpeg_encode_stream_u8(e._h, p["frames"], B, H, W, p["out"], cap, p["sizes"] + 1, p["total"]),
        "total+4": lambda p: lib().og_mjpeg_encode_stream_u8(e._h, p["frames"], B, H, W, p["out"], cap, p["sizes"], p["total"] + 4),
        "cap-1": lambda p: lib().og_mjpeg_encode_stream_u8(e._h, p["frames"], B, H, W, p["out"], cap - 1, p["sizes"], p["total"]),
    }
    for name, call in calls.items():
        rc, pay, faults = G.guarded_call(call, {"frames": c.frames}, {"out": cap, "sizes": 4 * B + 8, "total": 16})
        assert rc == OG_EINVAL and not faults, (name, faults)
        assert all((v == G.GUARD_FILL).all() for v in pay.values()), name
    blob, sizes = e.encode(c.frames)                                      # the handle stays usable
    assert blob.tobytes() == b"".join(MC.host_files("batch7"))
    print(G.report())
