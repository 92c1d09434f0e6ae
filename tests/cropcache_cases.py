"""Synthetic image / label pairs for the crop-training cache tests (tests/test_cropcache_host.py, tests/test_gpu_cropcache.py): six
PNG pairs of two shapes in runs A A B B A B, one label empty, and the best rows a detector could have given for them: one without a
detection and one sliver, one pixel high before padding."""
import hashlib
import io
import os

import numpy as np
from PIL import Image

SHAPES = ((64, 96), (64, 96), (80, 72), (80, 72), (64, 96), (80, 72))
EMPTY = 3                                                                     # the pair whose label holds no pixel
# x1 y1 x2 y2 conf in source pixels; -1: no detection
BEST = np.array([[20.7, 10.2, 70.9, 50.5, 0.9], [0.0, 0.0, 95.9, 63.9, 0.5], [-1, -1, -1, -1, -1], [3.5, 30.1, 70.2, 31.0, 0.8],
                 [60.3, 40.8, 96.0, 64.0, 0.7], [10.0, 12.0, 40.0, 70.0, 0.3]], np.float32)
NO_DETECTION, SLIVER = 2, 3


def pairs():
    """[(name, image [H,W,3] B G R, label [H,W])]"""
    out = []
    for i, (H, W) in enumerate(SHAPES):
        r = np.random.default_rng(40 + i)
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.clip(120 + 40 * np.sin(xx / 7.0 + i) + 30 * np.cos(yy / 5.0) + r.normal(0, 6, (H, W)), 0, 255)
        bgr = np.clip(img[..., None] + r.integers(-5, 6, (H, W, 3)), 0, 255).astype(np.uint8)
        lab = np.zeros((H, W), np.uint8)
        if i != EMPTY:
            cy, cx = H // 2 + 3 * i - 6, W // 2 - 4 * i + 9
            lab[((yy - cy) / (6.0 + i)) ** 2 + ((xx - cx) / (14.0 - i)) ** 2 <= 1.0] = 255 if i % 2 else 1      # label > 0, not only 255
        if i == 4:
            lab[0, :5] = 255                                                  # touches the top and the left border
        out.append((f"{100 + 7 * i}.png", bgr, lab))
    return out


def write(directory, suffix="_seg"):
    """the pairs as files: N.png (RGB) and N<suffix>.png (gray) -> (names, image paths, label paths)"""
    os.makedirs(directory, exist_ok=True)
    names, ips, lps = [], [], []
    for name, bgr, lab in pairs():
        ip, lp = os.path.join(directory, name), os.path.join(directory, name[:-4] + suffix + ".png")
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(ip)
        Image.fromarray(lab).save(lp)
        names.append(name)
        ips.append(ip)
        lps.append(lp)
    return names, ips, lps


class Rows:
    """a detector replaced by given best rows: called run by run, it hands them out in input order"""

    def __init__(self, rows=BEST):
        self.rows, self.at, self.calls = np.asarray(rows, np.float32), 0, []

    def __call__(self, frames, conf):
        n = len(frames)
        self.calls.append((n, tuple(frames.shape[1:]), float(conf)))
        out = self.rows[self.at:self.at + n].copy()
        out[out[:, 4] < conf] = -1
        self.at += n
        return out


def expected_boxes(roi, padding):
    """{input index: box} by the reference's lines, in numpy"""
    out = {}
    for i, (_, bgr, lab) in enumerate(pairs()):
        H, W = lab.shape
        if roi == "gt":
            if lab.max() == 0:
                continue
            ys, xs = np.where(lab > 0)
            b = (max(0, int(xs.min()) - padding), max(0, int(ys.min()) - padding), min(W, int(xs.max()) + 1 + padding), min(H, int(ys.max()) + 1 + padding))
        else:
            x1, y1, x2, y2, c = BEST[i]
            if c < 0.25:
                continue
            b = (max(0, int(x1) - padding), max(0, int(y1) - padding), min(W, int(x2) + padding), min(H, int(y2) + padding))
        if b[2] <= b[0] or b[3] <= b[1]:
            continue
        out[i] = b
    return out


def tree(directory):
    """{relative path: sha256} of every file below a directory"""
    out = {}
    for base, _, files in os.walk(directory):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, directory)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def gray_of(png_bytes_or_path):
    im = Image.open(io.BytesIO(png_bytes_or_path) if isinstance(png_bytes_or_path, bytes) else png_bytes_or_path)
    assert im.mode == "L"
    return np.asarray(im)
