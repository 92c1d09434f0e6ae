"""-m gpu: the device-touching entry points of include/openglottal_hip_sweep.h held to the buffer extents their callers declare
(tests/buffer_guard.py): guards untouched, every declared byte written, results independent of the slack around the inputs, inputs
unchanged, payloads bit-identical to the same call on plain buffers -- for one frame and for 70 frames in three micro-batches, at a
frame shape whose rows are no multiple of anything.  The host twin is held the same way in tests/test_sweep_host.py."""
import ctypes as C

import numpy as np
import pytest

import buffer_guard as G
import sweep_cases as S
import track_cases as T
from openglottal_amd import gated, sweep
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

# entry point -> the test of this module that puts it inside guards
SWEEP_MATRIX = {
    "og_sweep_counts_u8_dev": "test_resident_buffers",
    "og_sweep_counts_u8": "test_host_buffers",
    "og_sweep_get_state": "test_the_state",
}

H, W = 33, 257
THR = np.array([0.35, 0.5, 0.8], np.float64)
HOLD = np.array([0, 2, S.FOREVER], np.int32)
CN = len(THR) * len(HOLD)


def case(n):
    w = T.short_walk(70, 35, None, (H, W))
    pred, gt = S.masks_for((H, W), 70, 0.5)
    return pred[:n], gt[:n], w["best"][:n], w["resets"][:n]


def _run(entry, kind, n, chunk):
    pred, gt, best, resets = case(n)
    sw = sweep.Sweep()
    try:
        sw.set_chunk(chunk)
        fn = getattr(lib(), entry)
        for with_boxes in (True, False):
            for with_resets in (True, False):
                def call(p):
                    check(lib().og_sweep_reset(sw._h))
                    return fn(sw._h, p["pred"], p["gt"], p["best"], p["resets"], n, H, W, p["thr"], len(THR), p["hold"], len(HOLD), 30.0, 8, 0,
                              p["fc"], p["counts"], p["boxes"])
                out = G.run_guarded(entry, f"n={n} chunk={chunk} boxes={with_boxes} resets={with_resets}", call,
                                    {"pred": pred, "gt": gt, "best": best, "resets": resets if with_resets else None, "thr": THR, "hold": HOLD},
                                    {"fc": n * 12, "counts": CN * n * 12, "boxes": CN * n * 16 if with_boxes else None}, kind, sw.sync,
                                    input_kinds={"thr": "host", "hold": "host"})
                want = sweep.sweep_host(pred, gt, best, THR, HOLD, resets=resets if with_resets else None)
                assert np.array_equal(out["fc"].view(np.int32).reshape(n, 3), want["frame_counts"])
                assert np.array_equal(out["counts"].view(np.int32).reshape(CN, n, 3), want["counts"])
                if with_boxes:
                    assert np.array_equal(out["boxes"].view(np.int32).reshape(CN, n, 4), want["boxes"])
    finally:
        sw.close()


@pytest.mark.parametrize("n,chunk", [(1, 0), (70, 25)])
def test_resident_buffers(n, chunk):
    _run("og_sweep_counts_u8_dev", "device", n, chunk)


@pytest.mark.parametrize("n,chunk", [(1, 0), (70, 25)])
def test_host_buffers(n, chunk):
    _run("og_sweep_counts_u8", "host", n, chunk)


def test_the_state():
    pred, gt, best, resets = case(70)
    sw = sweep.Sweep()
    try:
        sw.counts(pred, gt, best, THR, HOLD, resets=resets)
        states = (gated.TrackState * CN)()
        sweep.sweep_host(pred, gt, best, THR, HOLD, resets=resets, states=states)
        for c in (0, 4, CN - 1):
            out = G.run_guarded("og_sweep_get_state", f"c={c}", lambda p: lib().og_sweep_get_state(sw._h, c, p["state"]), {}, {"state": 24})
            assert bytes(out["state"]) == bytes(states[c])
        st = gated.TrackState()
        assert lib().og_sweep_get_state(sw._h, CN, C.addressof(st)) == -1 and lib().og_sweep_get_state(sw._h, -1, C.addressof(st)) == -1
    finally:
        sw.close()


def test_the_matrix_names_every_entry_that_writes_a_callers_buffer():
    from openglottal_amd import _lib

    writers = {n for n in _lib.SWEEP_PROTOTYPES if n not in ("og_sweep_limit", "og_sweep_create", "og_sweep_destroy", "og_sweep_sync",
                                                             "og_sweep_set_chunk", "og_sweep_reset", "og_sweep_host", "og_sweep_plan")}
    assert writers == set(SWEEP_MATRIX) and all(name in globals() for name in SWEEP_MATRIX.values())
