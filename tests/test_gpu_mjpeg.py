"""-m gpu: the device's JPEG files against the host twin's, byte for byte, over the matrix of tests/mjpeg_cases.py: the resident entry
and the streamed one, at a micro-batch of 3 and at the default, twice."""
import numpy as np
import pytest
import torch

import mjpeg_cases as MC
from openglottal_amd import mjpeg as MJ

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def encoders():
    return {3: MJ.Mjpeg(chunk=3), 128: MJ.Mjpeg()}


def want(cid):
    files = MC.host_files(cid)
    return np.frombuffer(b"".join(files), np.uint8), np.array([len(j) for j in files], np.int32)


@pytest.mark.parametrize("cid", MC.IDS)
def test_both_entries_give_the_host_twins_bytes(encoders, cid):
    c = MC.BY_ID[cid]
    blob, sizes = want(cid)
    dev = torch.from_numpy(c.frames).to("cuda:0")
    for chunk, e in encoders.items():
        e.set_quality(c.quality)
        for attempt in range(2):
            got, gs = e.encode(c.frames)
            assert np.array_equal(gs, sizes), (chunk, attempt, gs, sizes)
            assert got.size == blob.size and np.array_equal(got, blob), (chunk, attempt, int(np.flatnonzero(got != blob)[0]))
            got, gs = e.encode_resident(dev)
            assert np.array_equal(gs, sizes), (chunk, attempt, gs, sizes)
            assert got.size == blob.size and np.array_equal(got, blob), (chunk, attempt, int(np.flatnonzero(got != blob)[0]))


def test_frames_at_any_address_and_a_changed_quality_on_one_handle(encoders):
    """The transform takes aligned dwords where a row allows it and bytes elsewhere: the same frames at the four byte offsets."""
    e = encoders[3]
    c = MC.BY_ID["batch7"]
    B, H, W = c.frames.shape[:3]
    for q in (75, 20, 75):
        e.set_quality(q)
        files = [MJ.encode_host(f, q) for f in c.frames]
        blob, sizes = np.frombuffer(b"".join(files), np.uint8), np.array([len(j) for j in files], np.int32)
        for off in range(4):
            raw = torch.zeros(c.frames.size + 8, dtype=torch.uint8, device="cuda:0")
            view = raw[off:off + c.frames.size].view(B, H, W, 3)
            view.copy_(torch.from_numpy(c.frames))
            got, gs = e.encode_resident(view)
            assert np.array_equal(gs, sizes) and np.array_equal(got, blob), (q, off)


def test_encode_resident_in_several_calls(encoders, monkeypatch):
    """`encode_resident` keeps its worst-case buffer to RESIDENT_CAP bytes: 7 frames as 2 + 2 + 2 + 1, and one frame larger than the cap"""
    c = MC.BY_ID["batch7"]
    blob, sizes = want("batch7")
    dev = torch.from_numpy(c.frames).to("cuda:0")
    e = encoders[3]
    e.set_quality(c.quality)
    for cap in (2 * MJ.bound(40, 56) + 5, 1):
        monkeypatch.setattr(MJ, "RESIDENT_CAP", cap)
        got, gs = e.encode_resident(dev)
        assert np.array_equal(gs, sizes) and np.array_equal(got, blob), cap


def test_an_empty_batch(encoders):
    blob, sizes = encoders[3].encode(np.zeros((0, 8, 8, 3), np.uint8))
    assert blob.size == 0 and sizes.size == 0
