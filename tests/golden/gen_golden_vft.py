"""Generate ``vft_guided.npz``: the reference's YOLO-guided VFT (pipeline 2) on three short synthetic videos.

Run on the build machine only (it needs the reference checkout next to the repository's build image, as gen_golden.py does):

    python tests/golden/gen_golden_vft.py

What runs is the reference's own, unmodified ``openglottal.models.tracker.YOLOGuidedVFT`` and
``openglottal.features.extract_features_yolo_guided_vft``, imported under the placeholder modules of gen_golden.py.  OpenCV is absent
from the build image, so the cv2 functions the tracker calls are provided here:

* ``findContours(RETR_EXTERNAL)`` / ``contourArea`` / ``drawContours(FILLED)`` as Moore border following from each component's
  raster-first pixel, the shoelace formula, and a winding-number polygon fill.  External contours are returned last-found-first
  (OpenCV's order from recall -- unpinned).  This is a different algorithm from the library's 2x2 windows and union-find, so the two
  restatements of ``_nblobs`` check each other.
* ``cvtColor(BGR2GRAY)``: OpenCV's published 15-bit fixed point (``openglottal_amd.utils.bgr_to_gray_numpy``).
* ``GaussianBlur`` / ``absdiff``: anything -- the tracker's motion map never reaches its output.  The fixture is generated twice,
  with two different blurs, and the two results are asserted equal.

The detector is scripted (``reset`` / ``detect``), ``load_frames_bgr`` is patched to return the synthetic frames.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

# clockwise from west, (dy, dx)
DIRS = [(0, -1), (-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1)]


def trace(m, sy, sx):
    """Moore border following of the component whose raster-first pixel is (sy, sx): closed list of (x, y), clockwise."""
    H, W = m.shape

    def on(y, x):
        return 0 <= y < H and 0 <= x < W and m[y, x]

    pts = [(sx, sy)]
    y, x, back = sy, sx, 0          # the pixel west of a raster-first pixel is background
    first = None
    while True:
        d = None
        for k in range(1, 9):
            c = (back + k) % 8
            if on(y + DIRS[c][0], x + DIRS[c][1]):
                d = c
                break
        if d is None:
            return pts                                   # an isolated pixel
        if (y, x) == (sy, sx):
            if first is None:
                first = d
            elif d == first:
                return pts[:-1]                          # back at the start, about to repeat the first move
        y, x = y + DIRS[d][0], x + DIRS[d][1]
        pts.append((x, y))
        back = (d - 2) % 8 if d % 2 == 0 else (d - 3) % 8


def polygon_fill(pts, H, W):
    """Pixels on the polygon through ``pts`` or with a nonzero winding number."""
    wn = np.zeros((H, W), np.int32)
    out = np.zeros((H, W), bool)
    xs = np.arange(W)
    for i, (x0, y0) in enumerate(pts):
        out[y0, x0] = True
        x1, y1 = pts[(i + 1) % len(pts)]
        if y1 > y0:
            wn[y0, xs < x0] += 1                         # rows [y0, y1): the row of the lower end, at that end's x
        elif y1 < y0:
            wn[y1, xs < x1] -= 1
    return out | (wn != 0)


def find_external(m):
    m = np.asarray(m) > 0
    H, W = m.shape
    owned = np.zeros((H, W), bool)
    seen = np.zeros((H, W), bool)
    found = []
    for y in range(H):
        for x in range(W):
            if not m[y, x] or seen[y, x]:
                continue
            stack = [(y, x)]                             # mark the component
            seen[y, x] = True
            while stack:
                cy, cx = stack.pop()
                for dy, dx in DIRS:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and m[ny, nx] and not seen[ny, nx]:
                        seen[ny, nx] = True
                        stack.append((ny, nx))
            if owned[y, x]:
                continue                                 # inside an outer contour found before: not external
            pts = trace(m, y, x)
            owned |= polygon_fill(pts, H, W)
            found.append(np.array(pts, np.int32).reshape(-1, 1, 2))
    return found[::-1]


def contour_area(c):
    """The shoelace formula over a contour as ``find_external`` returns it."""
    p = c.reshape(-1, 2).astype(np.int64)
    q = np.roll(p, -1, axis=0)
    return abs(int((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())) / 2.0


def install_cv2(blur):
    import gen_golden as G
    from openglottal_amd.utils import bgr_to_gray_numpy

    G.install_placeholders()
    cv2 = sys.modules["cv2"]
    cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE, cv2.FILLED = 0, 2, -1
    cv2.cvtColor = lambda img, code: bgr_to_gray_numpy(img)
    cv2.absdiff = lambda a, b: np.abs(a - b)
    cv2.GaussianBlur = blur
    cv2.findContours = lambda m, mode, method: (find_external(m), None)

    def draw_contours(img, contours, idx, color, thickness):
        assert idx == -1 and thickness == cv2.FILLED
        for c in contours:
            img[polygon_fill([tuple(v) for v in c.reshape(-1, 2)], *img.shape)] = color
        return img

    cv2.contourArea = contour_area
    cv2.drawContours = draw_contours
    return cv2


class ScriptedDetector:
    model = None

    def __init__(self, boxes):
        self.boxes, self.i = boxes, 0

    def reset(self):
        self.i = 0

    def detect(self, frame):
        b = self.boxes[self.i]
        self.i += 1
        return b


SEQUENCES = (("a", 31, 24, 64, 64), ("b", 32, 40, 32, 48), ("c", 33, 16, 64, 64))     # name, seed, frames, H, W
INIT = 2
NO_BOX = -(1 << 20)                                                                    # a row of this value: None


def run(blur):
    import classic_cases as K

    install_cv2(blur)
    for name in [k for k in sys.modules if k == "openglottal" or k.startswith("openglottal.")]:
        del sys.modules[name]
    import openglottal.features as F
    from openglottal.models.tracker import YOLOGuidedVFT

    out = {}
    for name, seed, n, H, W in SEQUENCES:
        frames, boxes = K.sequence(seed, n, H, W)
        if name == "c":
            boxes[0] = boxes[1] = None                   # no box among the init frames: the seed comes from the whole frame
        gray = [sys.modules["cv2"].cvtColor(f, 6) for f in frames]
        first = next((b for b in boxes[:INIT] if b is not None), None)
        tr = YOLOGuidedVFT(**F.YGVFT_PARAMS)
        tr.initialize(gray[:INIT], bbox=first)
        th, areas, masks = [tr.thresh], [], []
        for g, b in zip(gray[INIT:], boxes[INIT:]):
            m = tr.process_frame(g, b)
            th.append(tr.thresh)
            areas.append(int((m > 0).sum()))
            masks.append(np.packbits(m > 0))
        F.load_frames_bgr = lambda path, fr=frames: list(fr)
        feats = F.extract_features_yolo_guided_vft(name, ScriptedDetector(boxes), INIT)
        assert np.array_equal(feats["_area"], [0.0] * INIT + [float(a) for a in areas])
        F.load_frames_bgr = lambda path, fr=frames: list(fr[:INIT + 1])
        assert F.extract_features_yolo_guided_vft(name, ScriptedDetector(boxes), INIT) is None
        out[f"{name}_frames"] = frames
        out[f"{name}_boxes"] = np.array([[NO_BOX] * 4 if b is None else list(b) for b in boxes], np.int32)
        out[f"{name}_thresh"] = np.array(th, np.float64)                 # [0]: the seed; [1 + i]: after process frame i
        out[f"{name}_area"] = np.array(areas, np.int32)
        out[f"{name}_masks"] = np.stack(masks)
        out[f"{name}_feat_keys"] = np.array([k for k in feats if k != "_area"])
        out[f"{name}_feat_vals"] = np.array([np.nan if feats[k] is None else float(feats[k]) for k in feats if k != "_area"], np.float64)
    out["init"] = np.array(INIT)
    out["no_box"] = np.array(NO_BOX)
    out["too_short_is_none"] = np.array(True)
    return out


def main():
    a = run(lambda img, ksize, sigma: img.copy())
    b = run(lambda img, ksize, sigma: img * 0.25 + np.roll(img, 1, axis=0) * 0.5 + 3.0)
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), f"{k} depends on the blur"
    path = os.path.join(HERE, "vft_guided.npz")
    np.savez_compressed(path, **a)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; areas " + " ".join(f"{n}:{a[n + '_area'].tolist()}" for n, *_ in SEQUENCES))


if __name__ == "__main__":
    main()
