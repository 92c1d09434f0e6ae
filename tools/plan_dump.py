"""Every record of the launch plans (og_unet_plan, og_unet_plan_resized, og_yolo_plan) over a fixed matrix, on stdout.  No GPU.

For changes to the host launch layer that must not change a launch: run it on the build before and on the build after
(OPENGLOTTAL_HIP_LIB selects the library) and diff the two outputs.  The matrix is tests/test_launch_plan.py's, the opt-in
precisions and the forced direct kernels, the resized chain and the detector.  usage: python tools/plan_dump.py > plans.txt
"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_launch_plan as T  # noqa: E402
from oracle import yolo_layer_ref as YR  # noqa: E402
from openglottal_amd import synth  # noqa: E402
from openglottal_amd._lib import lib  # noqa: E402
from openglottal_amd.yolo import YoloPlanner  # noqa: E402

BATCHES = list(range(1, 65)) + [96, 128, 200, 256]
n_records = 0


def emit(what, n, text):
    global n_records
    assert n > 0, (what, n, lib().og_last_error())
    lines = text.decode().strip().split("\n")
    assert len(lines) == n, (what, n, len(lines))
    n_records += n
    print("#", *what)
    print("\n".join(lines))


def unet(feats, B, H, W, lanes, options, resized_from=None):
    f = (C.c_int * len(feats))(*feats)
    buf = C.create_string_buffer(1 << 20)
    if resized_from:
        sh, sw, ch = resized_from
        n = lib().og_unet_plan_resized(f, len(feats), B, sh, sw, ch, H, W, lanes, options.encode(), buf, len(buf), None)
    else:
        n = lib().og_unet_plan(f, len(feats), B, H, W, lanes, options.encode(), buf, len(buf), None)
    emit((feats, B, H, W, lanes, options, resized_from), n, buf.value)


def main():
    more = ["precision=2", "precision=2,h_square=0", "precision=2,tile_h=8", "precision=2,h_square=0,tile_h=8",
            "wino=0,conv_impl=0", "wino=0,entry_f32=1", "wino=0,tps_nt1=9,tps_nt2=3,conv_impl=1"]
    for options in T.OPTION_SETS + more:
        for B in BATCHES:
            for lanes in (1, 3):
                unet(T.FULL, B, 256, 256, lanes, options)
    for feats, (H, W) in T.test_other_nets_and_frame_shapes.pytestmark[0].args[1]:
        for options in ("", "wino_w=0", "wino_w=0,wino_ps=4", "wino_w=2", "wino_w=3", "wino_w=4", "wino=0,splitk=1"):
            for B in (1, 2, 3, 5, 11, 16, 33, 64):
                unet(feats, B, H, W, 1, options)
    for src in ((480, 640, 3), (1080, 1920, 1)):
        for B in (1, 5, 64):
            unet(T.FULL, B, 256, 256, 1, "", resized_from=src)
    P = YoloPlanner(synth.make_yolov8_state_dict(**YR.NETS["n"]))
    for options in ("precision=0", "precision=2"):
        for H, W in ((256, 256), (160, 256)):
            for B in (1, 2, 4, 5, 64, 256):
                text = P.plan_text(B, H, W, 0, options, want_arena=False)
                emit(("yolo", B, H, W, options), len(text.splitlines()), text.encode())
    print(f"{n_records} records", file=sys.stderr)


if __name__ == "__main__":
    main()
