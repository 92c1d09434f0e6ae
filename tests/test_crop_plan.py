"""og_unet_plan_crops: the micro-batches of og_unet_stream_crops_u8 walked without a device -- the boxes (host inputs) decide the
compaction, every launch is recorded with its grid, LDS, workspace and the ring-slot buffers it writes.  No GPU."""
import itertools

import numpy as np
import pytest

import crop_cases as K
from openglottal_amd._lib import lib

FEATS = (4, 8, 16, 32)
CHUNK = 4
GOOD = K.USABLE[1]
NONE = (-1, -1, -1, -1)


def boxes_for(pattern, B):
    rows = {"all": [GOOD] * B, "none": [NONE] * B, "alternating": [GOOD if i % 2 == 0 else NONE for i in range(B)],
            "sliver": [K.SLIVER if i == B // 2 else K.USABLE[i % len(K.USABLE)] for i in range(B)]}[pattern]
    usable = sum(1 for r in rows if r in K.USABLE)
    return np.array(rows, np.int32), usable


def micro_batches(recs):
    """Split the records at every k_crop_tiles launch (the first launch of a micro-batch)."""
    out = []
    for r in recs:
        if r["kernel"].startswith("k_crop_tiles"):
            out.append([])
        out[-1].append(r)
    return out


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "sliver"])
def test_the_plan_follows_the_compaction_and_every_launch_stays_inside_its_slot(pattern, channels):
    limit = lib().og_workspace_limit
    for B, lanes in itertools.product((1, 5, 23), (1, 2, 3)):
        boxes, n_usable = boxes_for(pattern, B)
        recs, arena = K.plan_crops(FEATS, B, K.H, K.W, channels, boxes, K.SIZE, lanes, f"chunk={CHUNK}")
        label = (pattern, channels, B, lanes)
        if n_usable == 0:
            assert recs == [], label         # nothing reaches the device
            continue
        mbs = micro_batches(recs)
        assert len(mbs) == -(-n_usable // CHUNK), label       # network chains = ceil(n_usable / chunk)
        left = n_usable
        for mb in mbs:
            nb = min(CHUNK, left)
            left -= nb
            assert mb[0]["kernel"] == f"k_crop_tiles<{channels}>" and mb[0]["grid"] == (-(-K.SIZE * K.SIZE // 256), nb, 1), (label, mb[0])
            assert mb[-1]["kernel"] == "k_crop_project<true>" and mb[-1]["grid"] == (-(-K.H * K.W // 256), nb, 1), (label, mb[-1])
            assert sum(1 for r in mb if r["kernel"].startswith("k_crop_")) == 2 and len(mb) > 4      # one chain between the two
            assert mb[-1]["writes"] == {"mask": nb * K.H * K.W, "area": 4 * nb}, (label, mb[-1])
            for r in mb:
                assert r["writes"].get("area", 0) <= 4 * nb and r["writes"].get("mask", 0) <= nb * K.H * K.W, (label, r)
                assert set(r["writes"]) <= {"mask", "area"}
                assert 1 <= r["grid"][0] and 1 <= r["grid"][1] <= limit(2) and 1 <= r["grid"][2] <= limit(2), (label, r)
                assert r["lds"] <= limit(3) and r["workspace"] <= limit(0) and r["counters"] <= limit(1) and r["block"] <= 1024, (label, r)
        assert left == 0


def test_arena_bytes_do_not_grow_with_the_video():
    for channels in (1, 3):
        a = {B: K.plan_crops(FEATS, B, K.H, K.W, channels, boxes_for("all", B)[0], K.SIZE, 2, f"chunk={CHUNK}")[1] for B in (1, 5, 23, 400)}
        assert a[5] == a[23] == a[400] and 0 < a[1] < a[5]
        # sparse detections: the arena is sized by the usable frames of a micro-batch, never above the all-usable figure
        sparse = K.plan_crops(FEATS, 23, K.H, K.W, channels, boxes_for("alternating", 23)[0], K.SIZE, 2, f"chunk={CHUNK}")[1]
        assert sparse == a[23]


def test_large_frames_lower_the_micro_batch_to_the_slot_cap():
    """64 MiB of source frames per slot: 4096 x 4096 BGR frames are 48 MiB each, so a micro-batch is one frame whatever the chunk."""
    B = 3
    boxes = np.array([(0, 0, 4096, 4096)] * B, np.int32)
    recs, _ = K.plan_crops(FEATS, B, 4096, 4096, 3, boxes, K.SIZE, 1, "chunk=32")
    mbs = micro_batches(recs)
    assert len(mbs) == B and all(mb[0]["grid"][1] == 1 and mb[-1]["writes"] == {"mask": 4096 * 4096, "area": 4} for mb in mbs)


def test_the_plan_refuses_what_the_engine_refuses():
    import ctypes as C

    feats = (C.c_int * 4)(*FEATS)
    out = C.create_string_buffer(1 << 16)
    boxes = np.array([GOOD], np.int32)
    call = lambda **k: lib().og_unet_plan_crops(feats, 4, k.get("B", 1), k.get("H", K.H), k.get("W", K.W), k.get("ch", 1), boxes.ctypes.data,
                                                k.get("size", K.SIZE), 1, k.get("opt", b""), out, k.get("cap", 1 << 16), None)
    assert call() > 0
    assert call(size=24) == -1 and b"2^n_levels" in lib().og_last_error()        # 24 is no multiple of 16
    assert call(ch=2) == -1 and call(H=0) == -1 and call(size=0) == -1 and call(B=0) == -1
    assert call(opt=b"chunk=0") == -1 and call(opt=b"no_such=1") == -1
    assert call(cap=8) == -1 and b"does not fit" in lib().og_last_error()
