"""-m gpu: the device-touching entry points of include/decode/openglottal_hip_mjpd.h held to the buffer extents their callers declare
(tests/buffer_guard.py): guards untouched, every declared byte written, results independent of the slack around the compressed bytes,
the inputs unchanged -- and the bytes equal to the host twin's."""
import ctypes as C

import numpy as np
import pytest

import buffer_guard as G
import mjpd_cases as DC
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import lib

pytestmark = pytest.mark.gpu

OG_EINVAL = -1
H, W = 17, 9


def files():
    return [DC.pillow_jpeg(H, W, form, 75, 1) for form in ("420",) * 2] + [DC.pillow_jpeg(H, W, "420", 30, 1, True, 1)]


def test_resident_entry():
    d = MJ.MjpegDecoder(chunk=2)
    blob, offsets, recs, tabs, form = MJ.records_host(files())
    d.set_tables(tabs, form["sampling"], form["Ri"])
    B = 3
    out = G.run_guarded("og_mjpd_decode_u8_dev", "17x9",
                        lambda p: lib().og_mjpd_decode_u8_dev(d._h, p["blob"], p["offsets"], p["recs"], B, H, W, p["frames"], B * H * W * 3, p["status"]),
                        {"blob": blob, "offsets": offsets, "recs": recs}, {"frames": B * H * W * 3, "status": 4 * B}, kind="device", sync=d.sync)
    assert not out["status"].view(np.int32).any()
    assert np.array_equal(out["frames"].reshape(B, H, W, 3), np.stack([DC.twin(j)[0] for j in files()]))


def test_streamed_entry():
    d = MJ.MjpegDecoder(chunk=2)
    blob, offsets = MJ._pack(files())
    B = 3
    hw = (C.c_int * 2)()
    out = G.run_guarded("og_mjpd_decode_stream", "17x9",
                        lambda p: lib().og_mjpd_decode_stream(d._h, p["blob"], p["offsets"], B, p["frames"], None, B * H * W * 3, p["status"],
                                                              C.addressof(hw), C.addressof(hw) + 4),
                        {"blob": blob, "offsets": offsets}, {"frames": B * H * W * 3, "status": 4 * B})
    assert (hw[0], hw[1]) == (H, W) and not out["status"].view(np.int32).any()
    assert np.array_equal(out["frames"].reshape(B, H, W, 3), np.stack([DC.twin(j)[0] for j in files()]))


def test_refusals_leave_all_guards_intact_and_the_handle_usable():
    d = MJ.MjpegDecoder(chunk=2)
    blob, offsets = MJ._pack(files())
    B, cap = 3, 3 * H * W * 3
    hw = (C.c_int * 2)()
    a = C.addressof(hw)
    calls = {
        "cap-1": lambda p: lib().og_mjpd_decode_stream(d._h, p["blob"], p["offsets"], B, p["frames"], None, cap - 1, p["status"], a, a + 4),
        "offsets+4": lambda p: lib().og_mjpd_decode_stream(d._h, p["blob"], p["offsets"] + 4, B, p["frames"], None, cap, p["status"], a, a + 4),
        "status+2": lambda p: lib().og_mjpd_decode_stream(d._h, p["blob"], p["offsets"], B, p["frames"], None, cap, p["status"] + 2, a, a + 4),
    }
    for name, call in calls.items():
        rc, pay, faults = G.guarded_call(call, {"blob": blob, "offsets": np.concatenate([offsets, offsets[-1:]])}, {"frames": cap, "status": 4 * B + 8})
        assert rc == OG_EINVAL and not faults, (name, faults)
        assert all((v == G.GUARD_FILL).all() for v in pay.values()), name
    _, _, recs, tabs, form = MJ.records_host(files())
    d.set_tables(tabs, form["sampling"], form["Ri"])
    dev = {
        "cap-1": lambda p: lib().og_mjpd_decode_u8_dev(d._h, p["blob"], p["offsets"], p["recs"], B, H, W, p["frames"], cap - 1, p["status"]),
        "offsets+4": lambda p: lib().og_mjpd_decode_u8_dev(d._h, p["blob"], p["offsets"] + 4, p["recs"], B, H, W, p["frames"], cap, p["status"]),
        "recs+2": lambda p: lib().og_mjpd_decode_u8_dev(d._h, p["blob"], p["offsets"], p["recs"] + 2, B, H, W, p["frames"], cap, p["status"]),
        "status+1": lambda p: lib().og_mjpd_decode_u8_dev(d._h, p["blob"], p["offsets"], p["recs"], B, H, W, p["frames"], cap, p["status"] + 1),
    }
    for name, call in dev.items():
        rc, pay, faults = G.guarded_call(call, {"blob": blob, "offsets": np.concatenate([offsets, offsets[-1:]]), "recs": np.concatenate([recs, recs[-1:]])},
                                         {"frames": cap, "status": 4 * B + 8}, kind="device", sync=d.sync)
        assert rc == OG_EINVAL and not faults, (name, faults)
        assert all((v == G.GUARD_FILL).all() for v in pay.values()), name
    assert np.array_equal(d.decode(files()), np.stack([DC.twin(j)[0] for j in files()]))      # the handle stays usable
    print(G.report())
