"""-m gpu: the host plumbing the streaming families share (csrc/og_stream.inc: the stream, OgBuf, the two-slot loop, the drain),
seen through each family's streamed entry.  ONE handle of overlay, mjpeg, mjpd (lane per interval, and split="auto"), classic
(Otsu) and sweep runs, at chunk 2:
  (a) 16 x 16 frames, B = 5: three micro-batches, both slots used twice, the last micro-batch ragged;
  (b) 40 x 24 frames, B = 3: every buffer grows while the handle has history;
  (c) (a) again: the larger buffers are kept;
  (d) a call that a host-side argument check refuses, then (a) again.
Every result equals a fresh handle's and the family's host twin, byte for byte; the refusal has the code and the message a fresh
handle gives.  No call here reaches the device with bad arguments."""
import ctypes as C

import numpy as np
import pytest

import mjpd_cases as DC
from openglottal_amd import classic as CL
from openglottal_amd import mjpeg as MJ
from openglottal_amd import overlay as OV
from openglottal_amd import sweep as SW
from openglottal_amd._lib import lib, ptr

pytestmark = pytest.mark.gpu

CHUNK = 2
SMALL, LARGE = (16, 16, 5), (40, 24, 3)      # H, W, B
OG_EINVAL = -1


def refusal(rc):
    return rc, lib().og_last_error().decode()


def boxes_for(H, W, B):
    """A box inside the frame, one that crosses its edge, none (the detector found nothing), in turn."""
    rows = [(2, 3, W - 3, H - 2), (-4, H // 2, W + 5, H + 9), None]
    return [rows[i % 3] for i in range(B)]


def blobs(H, W, B, seed):
    """Masks with holes and several components each."""
    return (np.random.RandomState(seed).rand(B, H, W) < 0.45).astype(np.uint8) * 255


class Overlay:
    def handle(self):
        return OV.Overlay(chunk=CHUNK)

    def inputs(self, H, W, B):
        return np.random.RandomState(H + B).randint(0, 256, (B, H, W, 3), dtype=np.uint8), blobs(H, W, B, 1), boxes_for(H, W, B)

    def run(self, h, x):
        return (h.annotate(x[0], x[1], x[2], "contour"),)      # outlined: the labelling's buffers are in use too

    def host(self, x):
        return (np.stack([OV.overlay_host(f, m, b, "contour") for f, m, b in zip(*x)]),)

    def refuse(self, h, x):
        B, H, W = x[0].shape[:3]
        return refusal(lib().og_overlay_stream_u8(h._h, ptr(x[0]), B, H, W, 3, ptr(x[1]), None, 1, None))      # out is null


class Mjpeg:
    def handle(self):
        return MJ.Mjpeg(quality=60, chunk=CHUNK)

    def inputs(self, H, W, B):
        return np.stack([DC.noise(H, W, seed=i) for i in range(B)])

    def run(self, h, x):
        return h.encode(x)

    def host(self, x):
        files = [np.frombuffer(MJ.encode_host(f, 60), np.uint8) for f in x]
        return np.concatenate(files), np.array([f.size for f in files], np.int32)

    def refuse(self, h, x):
        B, H, W = x.shape[:3]
        out, sizes, total = np.empty(B * MJ.bound(H, W), np.uint8), np.empty(B, np.int32), C.c_longlong()
        return refusal(lib().og_mjpeg_encode_stream_u8(h._h, ptr(x), B, H, W, ptr(out), out.size - 1, ptr(sizes), C.addressof(total)))


class Mjpd:
    """restart: MCUs per restart interval of the files (0: no markers, what split="auto" decodes with k_mjps_entropy)."""

    def __init__(self, split, form, restart):
        self.split, self.form, self.restart = split, form, restart

    def handle(self):
        return MJ.MjpegDecoder(chunk=CHUNK, split=self.split)

    def inputs(self, H, W, B):
        return [DC.pillow_jpeg(H, W, self.form, restart=self.restart, seed=i) for i in range(B)]

    def run(self, h, x):
        return h.decode(x, statuses=True)

    def host(self, x):
        twin = MJ.decode_split_host if self.split == "auto" else MJ.decode_host
        return np.stack([twin(j) for j in x]), np.zeros(len(x), np.int32)

    def refuse(self, h, x):
        blob, offsets = MJ._pack(x)
        info = MJ.parse(x[0])
        out, status, hw = np.empty((len(x), info["H"], info["W"], 3), np.uint8), np.zeros(len(x), np.int32), (C.c_int * 2)()
        return refusal(lib().og_mjpd_decode_stream(h._h, ptr(blob), ptr(offsets), len(x), ptr(out), None, out.size - 1, ptr(status),
                                                   C.addressof(hw), C.addressof(hw) + 4))


class Otsu:
    def handle(self):
        return CL.Classic(chunk=CHUNK)

    def inputs(self, H, W, B):
        return np.random.RandomState(H * B).randint(0, 256, (B, H, W), dtype=np.uint8), boxes_for(H, W, B)

    def run(self, h, x):
        return h.otsu_in_box(x[0], x[1])

    def host(self, x):
        gray, boxes = x
        B, H, W = gray.shape
        masks, areas, Ts = np.zeros((B, H, W), np.uint8), np.zeros(B, np.int32), np.zeros(B, np.int32)
        for i, b in enumerate(boxes):
            x1, y1, x2, y2 = CL.boxes_array([b], 1, W, H)[0]
            hist = CL.box_hist_host(gray[i], b)
            if x1 < 0 or not hist.any():
                continue
            Ts[i] = CL.otsu_threshold_host(hist)
            masks[i, y1:y2, x1:x2] = (gray[i, y1:y2, x1:x2] <= Ts[i]) * 255
            areas[i] = int((masks[i] > 0).sum())
        return masks, areas, Ts

    def refuse(self, h, x):
        B, H, W = x[0].shape
        bx, area = CL.boxes_array(x[1], B, W, H), np.zeros(B, np.int32)
        return refusal(lib().og_otsu_in_box_u8(h._h, ptr(x[0]), B, H, W, 1, ptr(bx), None, ptr(area), None))      # T is null


class Sweep:
    THR, HOLDS = [0.25, 0.5], [0, 3]

    def handle(self):
        h = SW.Sweep()
        h.set_chunk(CHUNK)
        return h

    def inputs(self, H, W, B):
        r = np.random.RandomState(H + W)
        x1, y1 = r.uniform(0, W / 2, B), r.uniform(0, H / 2, B)
        best = np.column_stack([x1, y1, x1 + r.uniform(1, W / 2, B), y1 + r.uniform(1, H / 2, B), r.uniform(0, 1, B)])      # xyxy, conf
        resets = np.zeros(B, np.uint8)
        resets[0] = 1                                                     # every call starts its trackers anew, on any handle
        return blobs(H, W, B, 2), blobs(H, W, B, 3), best.astype(np.float32), resets

    def run(self, h, x):
        got = h.counts(x[0], x[1], x[2], self.THR, self.HOLDS, resets=x[3])
        return got["frame_counts"], got["counts"], got["boxes"]

    def host(self, x):
        want = SW.sweep_host(x[0], x[1], x[2], self.THR, self.HOLDS, resets=x[3])
        return want["frame_counts"], want["counts"], want["boxes"]

    def refuse(self, h, x):
        B, H, W = x[0].shape
        t, hold = SW._grid(self.THR, self.HOLDS)
        fc, cnt = np.empty((B, 3), np.int32), np.empty((4, B, 3), np.int32)
        return refusal(lib().og_sweep_counts_u8(h._h, None, ptr(x[1]), ptr(x[2]), ptr(x[3]), B, H, W, ptr(t), 2, ptr(hold), 2, 30.0, 8, 0,
                                                ptr(fc), ptr(cnt), None))      # pred is null


FAMILIES = {"overlay": Overlay(), "mjpeg": Mjpeg(), "mjpd": Mjpd("off", "444", 2), "mjpd-split": Mjpd("auto", "420", 0), "otsu": Otsu(),
            "sweep": Sweep()}


def same(got, want, label):
    assert len(got) == len(want), label
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (label, i)


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_one_handle_through_growth_reuse_and_a_refusal(name):
    fam = FAMILIES[name]
    small, large = fam.inputs(*SMALL), fam.inputs(*LARGE)
    want = {"small": fam.host(small), "large": fam.host(large)}
    same(fam.run(fam.handle(), small), want["small"], (name, "fresh", "small"))      # the fresh handles: each equals the twin,
    same(fam.run(fam.handle(), large), want["large"], (name, "fresh", "large"))      # so the used one is compared with both at once
    used = fam.handle()
    for step, (x, key) in zip("abc", ((small, "small"), (large, "large"), (small, "small"))):
        same(fam.run(used, x), want[key], (name, step))
    refused = fam.refuse(used, small)
    assert refused[0] == OG_EINVAL and refused[1] and refused == fam.refuse(fam.handle(), small), (name, refused)
    same(fam.run(used, small), want["small"], (name, "d"))
