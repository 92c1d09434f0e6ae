"""-m gpu: og_aug_batch_u8_dev held to the buffer extents its caller declares (tests/buffer_guard.py): guards untouched, every output
byte written, results independent of the slack around the tiles, the indices and the records, the tiles unchanged -- and the bits
equal to the host twin's.  The case that matters most: the first and the last tile, rotated by +-30 degrees and enlarged, whose taps
next to the tile's border must read neither the neighbour tile nor the slack."""
import numpy as np
import pytest

import aug_cases as AC
import buffer_guard as G
from openglottal_amd import augment as A
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

OG_EINVAL = -1
KINDS = {"images": "device", "masks": "device", "idx": "device", "params": "host"}

# entry point -> the test of this module that puts it inside guards
AUG_MATRIX = {"og_aug_batch_u8_dev": "test_the_batch_entry_holds_its_extents"}


def entry(aug, N, S, b, augment=1):
    return lambda p: lib().og_aug_batch_u8_dev(aug._h, p["images"], p["masks"], N, S, p["idx"], p["params"], b, augment, p["out_img"], p["out_msk"])


def run(aug, S, idx, recs, label, augment=1):
    im, mk = AC.tiles(S)
    N, b = im.shape[0], len(idx)
    out = G.run_guarded("og_aug_batch_u8_dev", label, entry(aug, N, S, b, augment),
                        {"images": im, "masks": mk, "idx": np.asarray(idx, np.int32), "params": recs if augment else None},
                        {"out_img": 4 * b * S * S, "out_msk": 4 * b * S * S}, "device",
                        sync=lambda: check(lib().og_aug_sync(aug._h), "og_aug_sync"), input_kinds=KINDS)
    wi, wm = A.augment_host(im, mk, idx, recs, bool(augment))
    assert np.array_equal(out["out_img"].view(np.uint32), wi.reshape(-1).view(np.uint32)), label
    assert np.array_equal(out["out_msk"].view(np.float32), wm.reshape(-1)), label


@pytest.mark.parametrize("S", AC.SIZES)
def test_the_batch_entry_holds_its_extents(S):
    aug = A.Augmenter(S, chunk=3)
    N = AC.tiles(S)[0].shape[0]
    a = AC.angles(S)[1]
    edge = A.records([A.record(angle=s * a, new_size=int(1.15 * S), hflip=h, ks=5, blur_sigma=1.5) for s in (1, -1) for h in (False, True)])
    run(aug, S, [0, N - 1, N - 1, 0], edge, "first and last tile, rotated and enlarged")
    recs = AC.records(S)
    run(aug, S, [(c * 3) % N for c in range(len(recs))], recs, "the case list")
    run(aug, S, [N - 1, 0, N - 1], None, "plain", augment=0)


def test_refusals_leave_all_guards_intact_and_the_handle_usable():
    S = 32
    im, mk = AC.tiles(S)
    N, b = im.shape[0], 2
    aug = A.Augmenter(S, chunk=3)
    recs = A.records([A.record(angle=30), A.record(new_size=36)])
    bad = recs.copy()
    bad["new_size"][1] = 2 * S + 1
    nan = recs.copy()
    nan["cos_t"][0] = np.nan
    f = lib().og_aug_batch_u8_dev
    calls = {
        "idx+2": lambda p: f(aug._h, p["images"], p["masks"], N, S, p["idx"] + 2, p["params"], b, 1, p["out_img"], p["out_msk"]),
        "params+4": lambda p: f(aug._h, p["images"], p["masks"], N, S, p["idx"], p["params"] + 4, b, 1, p["out_img"], p["out_msk"]),
        "out_img+1": lambda p: f(aug._h, p["images"], p["masks"], N, S, p["idx"], p["params"], b, 1, p["out_img"] + 1, p["out_msk"]),
        "out_msk+2": lambda p: f(aug._h, p["images"], p["masks"], N, S, p["idx"], p["params"], b, 1, p["out_img"], p["out_msk"] + 2),
        "S=7": lambda p: f(aug._h, p["images"], p["masks"], N, 7, p["idx"], p["params"], b, 1, p["out_img"], p["out_msk"]),
        "S=1025": lambda p: f(aug._h, p["images"], p["masks"], N, 1025, p["idx"], p["params"], b, 1, p["out_img"], p["out_msk"]),
        "N=0": lambda p: f(aug._h, p["images"], p["masks"], 0, S, p["idx"], p["params"], b, 1, p["out_img"], p["out_msk"]),
        "b=-1": lambda p: f(aug._h, p["images"], p["masks"], N, S, p["idx"], p["params"], -1, 1, p["out_img"], p["out_msk"]),
        "no params": lambda p: f(aug._h, p["images"], p["masks"], N, S, p["idx"], None, b, 1, p["out_img"], p["out_msk"]),
        "no masks": lambda p: f(aug._h, p["images"], None, N, S, p["idx"], p["params"], b, 1, p["out_img"], p["out_msk"]),
    }
    for name, call in calls.items():
        rc, pay, faults = G.guarded_call(call, {"images": im, "masks": mk, "idx": np.array([0, N - 1], np.int32), "params": recs},
                                         {"out_img": 4 * b * S * S + 8, "out_msk": 4 * b * S * S + 8}, "device", input_kinds=KINDS)
        assert rc == OG_EINVAL and not faults, (name, faults)
        assert all((v == G.GUARD_FILL).all() for v in pay.values()), name
    for name, r in (("new_size", bad), ("cos_t", nan)):                        # a record outside the limits, named by its index
        rc, pay, faults = G.guarded_call(entry(aug, N, S, b), {"images": im, "masks": mk, "idx": np.array([0, N - 1], np.int32), "params": r},
                                         {"out_img": 4 * b * S * S, "out_msk": 4 * b * S * S}, "device", input_kinds=KINDS)
        assert rc == OG_EINVAL and not faults and name.encode() in lib().og_last_error(), name
        assert all((v == G.GUARD_FILL).all() for v in pay.values()), name
    run(aug, S, [0, N - 1], recs, "after the refusals")                        # the handle stays usable
    print(G.report())
