"""Every plan entry's text, byte for byte, against tests/golden/plan_texts.json.  The fixture records, per entry, the return value and
the text at two shapes -- one micro-batch, and a B that spans three micro-batches with a ragged last one where the entry walks
micro-batches (og_unet_plan and the detector's plan describe one chain) -- and the refusal of a buffer the text does not fit.
The texts are data: they were written by the library before the plan serializer was shared (og_plan_text, csrc/og_stream.inc), so a
change of a column, a separator or the refusal shows here.  No device.

Regenerate (only when a launch list changes on purpose): python tests/test_plan_text_golden.py --write"""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from openglottal_amd._lib import lib  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_texts.json")
FEATS = (4, 8, 16, 32)
SMALL_CAP = 8   # no plan text fits: the shortest line is longer

# name -> (entry, arguments before `out`); "/1": one micro-batch, "/3": three micro-batches, the last one ragged
CASES = {
    "og_unet_plan/1": ("og_unet_plan", (1, 64, 64, 1, b"")),
    "og_unet_plan/3": ("og_unet_plan", (5, 64, 96, 2, b"wino=0")),
    "og_unet_plan_resized/1": ("og_unet_plan_resized", (2, 48, 40, 3, 32, 32, 1, b"")),
    "og_unet_plan_resized/3": ("og_unet_plan_resized", (19, 2048, 4096, 1, 32, 32, 2, b"")),
    "og_unet_plan_crops/1": ("og_unet_plan_crops", (3, 96, 128, 1, 32, 1, b"chunk=4")),
    "og_unet_plan_crops/3": ("og_unet_plan_crops", (5, 96, 128, 3, 32, 2, b"chunk=2")),
    "og_classic_plan/1": ("og_classic_plan", (2, 16, 16, 1, 128)),
    "og_classic_plan/3": ("og_classic_plan", (5, 40, 24, 3, 2)),
    "og_classic_plan_tiled/1": ("og_classic_plan_tiled", (2, 16, 16, 1, 128, 2)),
    "og_classic_plan_tiled/3": ("og_classic_plan_tiled", (5, 300, 260, 3, 2, 1)),
    "og_overlay_plan/1": ("og_overlay_plan", (2, 16, 16, 1, 128, 1)),
    "og_overlay_plan/3": ("og_overlay_plan", (5, 40, 24, 3, 2, 2)),
    "og_mjpeg_plan/1": ("og_mjpeg_plan", (2, 16, 16, 128)),
    "og_mjpeg_plan/3": ("og_mjpeg_plan", (5, 40, 24, 2)),
    "og_mjpd_plan/1": ("og_mjpd_plan", (2, 16, 16, 1, 16, 128)),
    "og_mjpd_plan/3": ("og_mjpd_plan", (5, 40, 24, 3, 0, 2)),
    "og_mjps_plan/1": ("og_mjps_plan", (2, 16, 16, 1, 0, 128, 1, 0)),
    "og_mjps_plan/3": ("og_mjps_plan", (5, 40, 24, 3, 0, 2, 1, 64)),
    "og_yolo_plan/1": ("og_yolo_plan", (1, 64, 64, 0, b"")),
    "og_yolo_plan/3": ("og_yolo_plan", (5, 96, 64, 64, b"")),
}


@functools.lru_cache(maxsize=None)
def _planner():
    import decode_cases as DC
    from openglottal_amd.yolo import YoloPlanner

    return YoloPlanner(DC.base_sd())


def _call(entry, args, out, cap, bytes_ref):
    """The arguments in front of the ones the table gives: the feature list, the crops' boxes, the detector's handle."""
    if entry.startswith("og_unet_plan"):
        args = ((C.c_int * len(FEATS))(*FEATS), len(FEATS)) + tuple(args)
        if entry == "og_unet_plan_crops":
            boxes = np.ascontiguousarray(np.tile(np.array([8, 8, 72, 72], np.int32), (args[2], 1)))
            args = args[:6] + (boxes.ctypes.data,) + args[6:]
    elif entry == "og_yolo_plan":
        args = (_planner()._h,) + tuple(args)
    return getattr(lib(), entry)(*args, out, cap, bytes_ref)


def run(name):
    entry, args = CASES[name]
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong(-1)
    n = _call(entry, args, out, len(out), C.byref(ws))
    small = C.create_string_buffer(b"untouched", SMALL_CAP + 8)
    rc = _call(entry, args, small, SMALL_CAP, None)
    return {"ret": int(n), "text": out.value.decode(), "bytes": int(ws.value), "small_ret": int(rc),
            "small_error": lib().og_last_error().decode(), "small_out": small.value.decode()}


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES)
    for name, want in golden.items():
        assert want["ret"] == want["text"].count("\n") > 0, name
        assert want["small_ret"] < 0 and want["small_error"] == "plan text does not fit the buffer", name
        assert want["small_out"] == "untouched", name
    # the "/3" cases of the entries that walk micro-batches do span three, the last one ragged: the first kernel three times, its grid or workspace smaller last
    for entry in ("og_classic_plan", "og_classic_plan_tiled", "og_overlay_plan", "og_mjpeg_plan", "og_mjpd_plan", "og_mjps_plan",
                  "og_unet_plan_crops", "og_unet_plan_resized"):
        lines = golden[entry + "/3"]["text"].splitlines()
        grids = [ln.split("|")[1:8] for ln in lines if ln.split("|")[0] == lines[0].split("|")[0]]
        assert len(grids) == 3 and grids[0] == grids[1] != grids[2], (entry, grids)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_text_is_the_recorded_one(name, golden):
    assert run(name) == golden[name]


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    with open(FIXTURE, "w") as f:
        json.dump({name: run(name) for name in sorted(CASES)}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", FIXTURE)
