"""og_sweep_plan: the micro-batches and the workspace of a sweep, walked without a GPU.  The micro-batches tile N exactly, the default
chunk is max(1, min(4096, 256 MiB / (8 (H+1) (W+1)))), and the workspace is the header's formula:
min(chunk, N) * (8 (H+1) (W+1) + 16 n_conf n_hold) bytes."""
import ctypes as C

import pytest

from openglottal_amd import sweep
from openglottal_amd._lib import lib

NS = [0, 1, 4096, 4097, 10000]
SHAPES = [(256, 256), (2048, 2048), (1, 1)]


def default_chunk(H, W):
    return max(1, min(4096, (256 << 20) // (8 * (H + 1) * (W + 1))))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("N", NS)
def test_the_micro_batches_tile_n_and_the_workspace_is_the_formula(N, shape):
    H, W = shape
    for n_conf, n_hold in ((1, 1), (10, 22), (32, 32)):
        for chunk in (0, 1, 100, 4096):
            if chunk == 1 and N > 4097:
                continue
            mbs, ws = sweep.plan(N, H, W, n_conf, n_hold, chunk)
            eff = chunk or default_chunk(H, W)
            assert [b0 for b0, _ in mbs] == list(range(0, N, eff))
            assert all(1 <= nb <= eff for _, nb in mbs) and sum(nb for _, nb in mbs) == N
            assert all(nb == eff for _, nb in mbs[:-1])
            assert ws == min(eff, N) * (8 * (H + 1) * (W + 1) + 16 * n_conf * n_hold)


def test_the_default_chunks():
    assert default_chunk(256, 256) == 508 and default_chunk(2048, 2048) == 7 and default_chunk(1, 1) == 4096
    assert default_chunk(1, 4194304) == 3 and default_chunk(4194304, 1) == 3          # the largest frames: (H+1)(W+1) is just over 2 H W
    assert sweep.plan(5, 1, 4194304, 1, 1)[0] == [(0, 3), (3, 2)]
    assert len(sweep.plan(2000, 256, 256, 10, 22)[0]) == 4


def test_the_plan_refuses_what_the_entries_refuse():
    l = lib()
    out = C.create_string_buffer(1 << 16)
    ws = C.c_longlong()
    ok = (10, 8, 8, 2, 3, 0)
    assert l.og_sweep_plan(*ok, out, len(out), C.byref(ws)) == 1 and out.value == b"0|10\n"
    assert l.og_sweep_plan(*ok, out, len(out), None) == 1
    for bad in ((-1, 8, 8, 2, 3, 0), (10, 0, 8, 2, 3, 0), (10, 1, 4194305, 2, 3, 0), (10, 8, 8, 0, 3, 0), (10, 8, 8, 33, 3, 0),
                (10, 8, 8, 2, 0, 0), (10, 8, 8, 2, 33, 0), (10, 8, 8, 2, 3, -1), (10, 8, 8, 2, 3, 4097)):
        assert l.og_sweep_plan(*bad, out, len(out), C.byref(ws)) == -1, bad
    assert l.og_sweep_plan(*ok, None, 16, C.byref(ws)) == -1 and l.og_sweep_plan(*ok, out, 0, C.byref(ws)) == -1
    assert l.og_sweep_plan(10000, 8, 8, 2, 3, 1, out, 64, C.byref(ws)) == -1       # the text does not fit
    assert b"does not fit" in l.og_last_error()
