"""-m gpu: the device-touching entry points of include_ext/openglottal_hip_png.h held to the buffer extents their callers declare
(tests/buffer_guard.py): guards untouched, every declared byte written -- file i's pixels exactly in [offset_i, offset_i + H W C) --
results independent of the slack around the compressed bytes, the inputs unchanged, and the bytes equal to the host twin's."""
import numpy as np
import pytest

import buffer_guard as G
import png_cases as PC
from openglottal_amd import png as P
from openglottal_amd._lib import lib
from openglottal_amd.mjpeg import _pack

pytestmark = pytest.mark.gpu

OG_EINVAL = -1


def files():
    """mixed sizes and forms, a damaged file (zeros) and a refused one (no bytes) between good ones"""
    bad = dict((n, f) for n, f, _ in PC.hand_made_invalid())
    return [PC.simple(9, 17, 2, 8, None, 1), PC.simple(66, 5, 3, 4, None, 2), bad["adler"], PC.simple(3, 70, 0, 8, None, 3), bad["sixteen-bit"],
            PC.simple(7, 7, 6, 8, None, 4), bad["filter-type-5"]]


def want(C):
    tw = [P.decode_host(f, C, statuses=True) for f in files()]
    return np.concatenate([p.reshape(-1) for p, _ in tw if p is not None]), [s for _, s in tw]


@pytest.mark.parametrize("C", [3, 1])
def test_streamed_entry(C):
    d = P.PngDecoder(chunk=3)
    blob, offsets = _pack(files())
    B = len(files())
    px, st = want(C)
    out = G.run_guarded("og_png_decode_stream", f"mixed C={C}",
                        lambda p: lib().og_png_decode_stream(d._h, p["blob"], p["offsets"], B, C, p["out"], None, px.size, p["out_offsets"], p["hw"],
                                                             p["status"]),
                        {"blob": blob, "offsets": offsets}, {"out": px.size, "out_offsets": 8 * (B + 1), "hw": 8 * B, "status": 4 * B})
    assert out["status"].view(np.int32).tolist() == st == [0, 0, 5, 0, 6, 0, 7]
    assert np.array_equal(out["out"], px)
    assert out["out_offsets"].view(np.int64)[-1] == px.size and out["hw"].view(np.int32).reshape(B, 2)[4].tolist() == [0, 0]


def test_resident_entry():
    d = P.PngDecoder()
    r = P.records_host(files())
    d.set_palettes(r["pals"])
    B = len(files())
    px, st = want(3)
    assert r["out_bytes"] == px.size
    out = G.run_guarded("og_png_decode_u8_dev", "mixed",
                        lambda p: lib().og_png_decode_u8_dev(d._h, p["zblob"], p["zoffsets"], p["recs"], B, 3, r["raw_bytes"], r["max_pixels"], p["out"],
                                                             px.size, p["status"]),
                        {"zblob": r["zblob"], "zoffsets": r["zoffsets"], "recs": r["recs"]}, {"out": px.size, "status": 4 * B}, kind="device", sync=d.sync)
    assert out["status"].view(np.int32).tolist() == st and np.array_equal(out["out"], px)


def test_a_record_that_leaves_the_buffers_is_refused_and_writes_nothing():
    """cap one byte short of the last file: status 6 and not a byte of it written; raw bytes that leave the workspace: status 6 and zeros"""
    d = P.PngDecoder()
    good = [PC.simple(9, 17, 2, 8, None, 1), PC.simple(5, 6, 0, 8, None, 2), PC.simple(4, 4, 2, 8, None, 3)]
    r = P.records_host(good)
    d.set_palettes(r["pals"])
    px = np.concatenate([P.decode_host(f).reshape(-1) for f in good])
    recs = r["recs"].copy()
    recs["raw_offset"][1] = r["raw_bytes"] - 5 * 7 + 1
    rc, pay, faults = G.guarded_call(lambda p: lib().og_png_decode_u8_dev(d._h, p["zblob"], p["zoffsets"], p["recs"], 3, 3, r["raw_bytes"], r["max_pixels"],
                                                                         p["out"], px.size - 1, p["status"]),
                                     {"zblob": r["zblob"], "zoffsets": r["zoffsets"], "recs": recs}, {"out": px.size - 1, "status": 12}, kind="device",
                                     sync=d.sync)
    assert rc == 0 and not faults, faults
    assert pay["status"].view(np.int32).tolist() == [0, 6, 6]
    n0 = 9 * 17 * 3
    assert np.array_equal(pay["out"][:n0], px[:n0]) and not pay["out"][n0:n0 + 90].any() and (pay["out"][n0 + 90:] == G.GUARD_FILL).all()


def test_refusals_leave_all_guards_intact_and_the_handle_usable():
    d = P.PngDecoder(chunk=2)
    blob, offsets = _pack(files())
    B = len(files())
    px, st = want(3)
    cap = px.size
    outs = {"out": cap, "out_offsets": 8 * (B + 1) + 8, "hw": 8 * B + 8, "status": 4 * B + 8}
    calls = {
        "cap-1": lambda p: lib().og_png_decode_stream(d._h, p["blob"], p["offsets"], B, 3, p["out"], None, cap - 1, p["out_offsets"], p["hw"], p["status"]),
        "channels-2": lambda p: lib().og_png_decode_stream(d._h, p["blob"], p["offsets"], B, 2, p["out"], None, cap, p["out_offsets"], p["hw"], p["status"]),
        "offsets+4": lambda p: lib().og_png_decode_stream(d._h, p["blob"], p["offsets"] + 4, B, 3, p["out"], None, cap, p["out_offsets"], p["hw"], p["status"]),
        "out_offsets+4": lambda p: lib().og_png_decode_stream(d._h, p["blob"], p["offsets"], B, 3, p["out"], None, cap, p["out_offsets"] + 4, p["hw"], p["status"]),
        "hw+2": lambda p: lib().og_png_decode_stream(d._h, p["blob"], p["offsets"], B, 3, p["out"], None, cap, p["out_offsets"], p["hw"] + 2, p["status"]),
        "status+2": lambda p: lib().og_png_decode_stream(d._h, p["blob"], p["offsets"], B, 3, p["out"], None, cap, p["out_offsets"], p["hw"], p["status"] + 2),
        "no-place": lambda p: lib().og_png_decode_stream(d._h, p["blob"], p["offsets"], B, 3, None, None, cap, p["out_offsets"], p["hw"], p["status"]),
    }
    for name, call in calls.items():
        rc, pay, faults = G.guarded_call(call, {"blob": blob, "offsets": np.concatenate([offsets, offsets[-1:]])}, outs)
        assert rc == OG_EINVAL and not faults, (name, faults)
        assert all((v == G.GUARD_FILL).all() for v in pay.values()), name
    r = P.records_host(files())
    d.set_palettes(r["pals"])
    ins = {"zblob": r["zblob"], "zoffsets": np.concatenate([r["zoffsets"], r["zoffsets"][-1:]]), "recs": np.concatenate([r["recs"], r["recs"][-1:]])}
    args = lambda p, **k: [d._h, p["zblob"], k.get("zo", p["zoffsets"]), k.get("recs", p["recs"]), k.get("B", B), k.get("C", 3),   # noqa: E731
                           k.get("raw", r["raw_bytes"]), k.get("mp", r["max_pixels"]), p["out"], cap, k.get("st", p["status"])]
    dev = {
        "zoffsets+4": lambda p: lib().og_png_decode_u8_dev(*args(p, zo=p["zoffsets"] + 4)),
        "recs+4": lambda p: lib().og_png_decode_u8_dev(*args(p, recs=p["recs"] + 4)),
        "status+1": lambda p: lib().og_png_decode_u8_dev(*args(p, st=p["status"] + 1)),
        "channels-4": lambda p: lib().og_png_decode_u8_dev(*args(p, C=4)),
        "raw-negative": lambda p: lib().og_png_decode_u8_dev(*args(p, raw=-1)),
        "max-pixels-0": lambda p: lib().og_png_decode_u8_dev(*args(p, mp=0)),
        "B-negative": lambda p: lib().og_png_decode_u8_dev(*args(p, B=-1)),
    }
    for name, call in dev.items():
        rc, pay, faults = G.guarded_call(call, ins, {"out": cap, "status": 4 * B + 8}, kind="device", sync=d.sync)
        assert rc == OG_EINVAL and not faults, (name, faults)
        assert all((v == G.GUARD_FILL).all() for v in pay.values()), name
    got, status = d.decode(files(), statuses=True)                            # the handle stays usable
    assert status.tolist() == st and np.array_equal(np.concatenate([g.reshape(-1) for g in got]), px)
    print(G.report())
