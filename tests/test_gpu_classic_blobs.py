"""-m gpu: k_blobs (raw mask, hole fill, labelling, keys, top-n, paint, count: one workgroup per frame) through
og_vft_guided_u8_dev against og_blobs_host, on the named masks of tests/classic_cases.py and on batches that cross a micro-batch
boundary.  beta = 1 keeps the threshold at 128 (1.0 * t + 0.0 * cur), the box covers the frame and the frame is 0 where the mask is
set and 255 elsewhere, so the raw mask of the kernel IS the given mask.  Equality everywhere; every shape runs twice."""
import numpy as np
import pytest
import torch

import classic_cases as K
from openglottal_amd import classic as CL

pytestmark = pytest.mark.gpu

_ENG = {}


def engine(n):
    if n not in _ENG:
        e = CL.Classic(beta=1.0, percentile=30, n_components=n)
        e.thresh = 128.0
        _ENG[n] = e
    return _ENG[n]


def run_dev(masks, n, chunk=32):
    """masks [B,H,W] {0,1} -> (mask [B,H,W], area [B]) from the resident entry."""
    e = engine(n)
    e.set_chunk(chunk)
    B, H, W = masks.shape
    frames = torch.from_numpy(np.where(masks > 0, 0, 255).astype(np.uint8)).cuda()
    boxes = torch.tensor([[0, 0, W, H]] * B, dtype=torch.int32).cuda()
    out = torch.full((B, H, W), 7, dtype=torch.uint8, device="cuda")
    area = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    th = torch.zeros(B, dtype=torch.float64, device="cuda")
    e.guided_vft_dev(frames, B, H, W, 1, boxes, area, out, th)
    e.sync()
    assert (th.cpu().numpy() == 128.0).all()
    return out.cpu().numpy(), area.cpu().numpy()


_HOST = {}


def host(m, n):
    key = (m.tobytes(), m.shape, n)
    if key not in _HOST:
        _HOST[key] = CL.blobs_host(m, n)
    return _HOST[key]


@pytest.mark.parametrize("n", K.NS)
def test_named_masks_equal_the_host_twin(n):
    by_shape = {}
    for name, m in K.named_masks():
        by_shape.setdefault(m.shape, []).append((name, m))
    for shape, group in by_shape.items():
        batch = np.stack([m for _, m in group])
        got = run_dev(batch, n)
        again = run_dev(batch, n)
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1]), shape       # the same bits twice
        for i, (name, m) in enumerate(group):
            want_mask, want_area = host(m, n)
            assert got[1][i] == want_area and np.array_equal(got[0][i], want_mask), (name, n, int(got[1][i]), want_area)


@pytest.mark.parametrize("B,chunk", [(1, 32), (3, 2), (70, 32)])
def test_batches_across_a_micro_batch_boundary(B, chunk):
    rs = np.random.RandomState(100 + B)
    dens = rs.choice([0.3, 0.5, 0.6], B)
    masks = (rs.rand(B, 32, 48) < dens[:, None, None]).astype(np.uint8)
    got = run_dev(masks, 2, chunk)
    again = run_dev(masks, 2, chunk)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    for i in range(B):
        want_mask, want_area = host(masks[i], 2)
        assert got[1][i] == want_area and np.array_equal(got[0][i], want_mask), i


@pytest.mark.parametrize("B,H,W", [(8, 256, 256), (2, 120, 160)])
def test_larger_frames(B, H, W):
    """More pixels than one pass of the workgroup: smooth blobs with holes and specks, as a thresholded frame looks."""
    rs = np.random.RandomState(H)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for _ in range(4):
            cy, cx, ry, rx = rs.randint(20, H - 20), rs.randint(20, W - 20), rs.randint(5, 30), rs.randint(5, 40)
            d = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2
            masks[b][(d < 1) & (d > 0.2 * (b % 3))] = 1
        masks[b][rs.rand(H, W) < 0.01] ^= 1
    got = run_dev(masks, 2)
    again = run_dev(masks, 2)
    assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
    for b in range(B):
        want_mask, want_area = host(masks[b], 2)
        assert got[1][b] == want_area and np.array_equal(got[0][b], want_mask), b
    assert got[1].min() > 0
