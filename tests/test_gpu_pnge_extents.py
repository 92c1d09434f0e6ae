"""-m gpu: the device-touching entry points of include_enc/openglottal_hip_pnge.h held to the buffer extents their callers declare
(tests/buffer_guard.py): guards untouched, nothing written at or past out[total], sizes and total written whole, results independent
of the slack around the frames, the frames unchanged -- and the bytes equal to the host twin's.  `out` is declared at its capacity
and filled only up to `total`, so, as in tests/test_gpu_mjpeg_extents.py, the single guarded runs apply."""
import numpy as np
import pytest

import buffer_guard as G
import pnge_cases as EC
from openglottal_amd import png as P
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

OG_EINVAL = -1
CASES = ("seam-rows-c3-s64", "noise-c1-s256", "runs-c1-s32768", "two-segments-181x182-c1-s32768", "raw-S+1-64-c1-s64")

# entry point -> the test of this module that puts it inside guards
PNGE_MATRIX = {
    "og_pnge_encode_u8_dev": "test_resident_frames",
    "og_pnge_encode_stream_u8": "test_host_streaming",
}


def held(entry, kind, cid, sync=None):
    frames, S = EC.batch(cid), EC.by_id(cid)[2]
    B, H, W, C = frames.shape
    files = EC.host_files(cid)
    want = np.frombuffer(b"".join(files), np.uint8)
    cap = B * P.encode_bound(H, W, C, S)
    e = P.PngEncoder(chunk=3, segment=S)
    for slack in (0x00, 0xFF):
        rc, pay, faults = G.guarded_call(lambda p: entry(e._h, p["frames"], B, H, W, C, p["out"], cap, p["sizes"], p["total"]),
                                         {"frames": frames}, {"out": cap, "sizes": 4 * B, "total": 8}, kind,
                                         sync=(lambda: check(lib().og_pnge_sync(e._h), "og_pnge_sync")) if sync else None, slack=slack)
        assert rc == 0 and not faults, (cid, slack, faults)
        total = int(pay["total"].view(np.int64)[0])
        assert total == want.size and pay["sizes"].view(np.int32).tolist() == [len(f) for f in files], cid
        assert np.array_equal(pay["out"][:total], want), cid
        assert (pay["out"][total:] == G.GUARD_FILL).all(), (cid, "written past total")
        G.CASES[entry.__name__] += 1


@pytest.mark.parametrize("cid", CASES)
def test_host_streaming(cid):
    held(lib().og_pnge_encode_stream_u8, "host", cid)


@pytest.mark.parametrize("cid", CASES)
def test_resident_frames(cid):
    held(lib().og_pnge_encode_u8_dev, "device", cid, sync=True)


def test_refusals_leave_all_guards_intact_and_the_handle_usable():
    cid = "seam-rows-c3-s64"
    frames = EC.batch(cid)
    B, H, W, C = frames.shape
    cap = B * P.encode_bound(H, W, C, 64)
    e = P.PngEncoder(chunk=3, segment=64)
    stream, dev = lib().og_pnge_encode_stream_u8, lib().og_pnge_encode_u8_dev
    calls = {
        "sizes+1": ("host", lambda p: stream(e._h, p["frames"], B, H, W, C, p["out"], cap, p["sizes"] + 1, p["total"])),
        "total+4": ("host", lambda p: stream(e._h, p["frames"], B, H, W, C, p["out"], cap, p["sizes"], p["total"] + 4)),
        "cap-1": ("host", lambda p: stream(e._h, p["frames"], B, H, W, C, p["out"], cap - 1, p["sizes"], p["total"])),
        "cap-1 resident": ("device", lambda p: dev(e._h, p["frames"], B, H, W, C, p["out"], cap - 1, p["sizes"], p["total"])),
        "C=2": ("host", lambda p: stream(e._h, p["frames"], B, H, W, 2, p["out"], cap, p["sizes"], p["total"])),
    }
    for name, (kind, call) in calls.items():
        rc, pay, faults = G.guarded_call(call, {"frames": frames}, {"out": cap, "sizes": 4 * B + 8, "total": 16}, kind)
        assert rc == OG_EINVAL and not faults, (name, faults)
        assert all((v == G.GUARD_FILL).all() for v in pay.values()), name
    assert b"".join(e.files(frames)) == b"".join(EC.host_files(cid))          # the handle stays usable
    print(G.report())
