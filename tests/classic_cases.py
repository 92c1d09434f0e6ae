"""Helper module of the classical-family tests (tests/test_classic_host.py, tests/test_gpu_classic_*.py): the named masks of the blob
filter, the hard masks at any side (spiral, serpentine, nested rings, ...) and the window cases built from them, an independent
scipy statement of the filter, the contour statement the fixture's generator uses, and a numpy statement of the Otsu rule."""
import numpy as np

NS = (1, 2, 3, 8)


def _canvas(h, w):
    return np.zeros((h, w), np.uint8)


def spiral(S):
    """A square spiral walking inward from (0, 0), one pixel wide with a one-pixel channel: ONE 8-connected component (one long
    union chain) whose background is ONE 4-connected component, open to the border at (1, 0) -- no hole.  The walker turns right
    when the next pixel is outside or set, or the one after it is set (that keeps the channel); it stops when it cannot move
    after a turn (at an even side the last steps close a 2 x 2 end in the centre).  S * (S + 2) / 2 pixels at an even side."""
    m = _canvas(S, S)

    def can(y, x, dy, dx):
        ny, nx, ay, ax = y + dy, x + dx, y + 2 * dy, x + 2 * dx
        if not (0 <= ny < S and 0 <= nx < S) or m[ny, nx]:
            return False
        return not (0 <= ay < S and 0 <= ax < S and m[ay, ax])

    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    while True:
        if not can(y, x, dy, dx):
            dy, dx = dx, -dy
            if not can(y, x, dy, dx):
                return m
        y, x = y + dy, x + dx
        m[y, x] = 1


def hard_masks(S):
    """(name, mask u8 {0,1}) pairs at side S, the shapes a union-find labelling is slowest or most contended on; each also
    transposed (``-T``), rotated by 180 degrees (``-rot``) and inverted (``-inv``)."""
    yy, xx = np.indices((S, S))
    base = [("spiral", spiral(S))]
    serp = _canvas(S, S)                   # full rows on even lines, joined alternately at the right and the left end
    serp[0::2] = 1
    for y in range(1, S - 1, 2):
        serp[y, S - 1 if (y // 2) % 2 == 0 else 0] = 1
    base.append(("serpentine", serp))
    rings = _canvas(S, S)                  # concentric one-pixel square rings two apart: a hole in a hole in a hole
    for o in range(0, (S + 1) // 2, 2):
        rings[o, o:S - o] = rings[S - 1 - o, o:S - o] = 1
        rings[o:S - o, o] = rings[o:S - o, S - 1 - o] = 1
    base.append(("rings", rings))
    base.append(("specks", ((yy % 2 == 0) & (xx % 2 == 0)).astype(np.uint8)))       # key 0 each: the tie rule alone orders them
    base.append(("stairs", ((yy + xx) % 3 == 0).astype(np.uint8)))                  # chains 8-connected by diagonal steps only
    base.append(("checkerboard", ((yy + xx) % 2).astype(np.uint8)))
    comb = _canvas(S, S)
    comb[S - 2, 1:S - 1] = 1
    comb[0:S - 2, 1:S - 1:2] = 1
    base.append(("comb", comb))
    out = []
    for name, m in base:
        out += [(name, m), (name + "-T", np.ascontiguousarray(m.T)), (name + "-rot", np.ascontiguousarray(m[::-1, ::-1])),
                (name + "-inv", (1 - m).astype(np.uint8))]
    return out


WINDOW_FRAME = (40, 56)                    # H, W of the frames of the window cases
WINDOW_AT = (4, 11)                        # the 33 x 33 hard masks sit at rows 4:37, columns 11:44
WINDOW_BOXES = (
    (11, 4, 44, 37), (0, 0, 56, 40),                                             # the square, the frame
    (0, 0, 30, 20), (26, 0, 56, 20), (0, 20, 30, 40), (26, 20, 56, 40),          # the four corners: two frame edges each
    (0, 10, 30, 30), (20, 0, 40, 40),                                            # one edge; top and bottom
    (12, 5, 13, 36), (11, 20, 44, 21), (20, 20, 21, 21),                         # one column, one row, one pixel
    (10, 3, 45, 38), (12, 5, 43, 36),                                            # one pixel larger, one pixel smaller than the square
    (-45, -36, -12, -3),                                                         # counted from the far edge
    (30, 30, 90, 70),                                                            # leaves the frame
)


def window_cases():
    """(name, mask [40,56] u8 {0,1}) pairs: every 33 x 33 hard mask inside the frame, once with nothing set outside the square and
    once (``+dark``) with EVERYTHING outside it set -- whatever of that lies outside a box must be ignored."""
    H, W = WINDOW_FRAME
    y0, x0 = WINDOW_AT
    out = []
    for name, m in hard_masks(33):
        for dark in (0, 1):
            f = np.full((H, W), dark, np.uint8)
            f[y0:y0 + 33, x0:x0 + 33] = m
            out.append((name + ("+dark" if dark else ""), f))
    return out


def roi_of(box, H, W):
    """The pixels of ``m[y1:y2, x1:x2]`` (Python slices) as a bool [H,W]; nothing for ``None``."""
    roi = np.zeros((H, W), bool)
    if box is not None:
        roi[box[1]:box[3], box[0]:box[2]] = True
    return roi


LADDER_SIDES = (32, 64, 128, 256)          # the worst case climbs these, smallest first
LADDER_MASKS = ("spiral", "spiral-T", "serpentine", "rings")
LADDER_LIMIT_S = 2.0                       # no rung is launched whose predicted time exceeds this


def ladder_masks(S):
    by = dict(hard_masks(S))
    return [(name, by[name]) for name in LADDER_MASKS]


def ladder_prediction(times):
    """The time to expect of the next rung (the side doubles: four times the pixels) from the rungs already run: the last time
    times the last growth factor, at least 4."""
    growth = times[-1] / times[-2] if len(times) > 1 and times[-2] > 0 else 4.0
    return times[-1] * max(4.0, growth)


_SCIPY = {}


def scipy_blobs_cached(mask, n):
    """``scipy_blobs`` computed once per (mask, n) and shared among the tests of a run; the arrays are read-only."""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    key = (m.tobytes(), m.shape, n)
    if key not in _SCIPY:
        out, area = scipy_blobs(m, n)
        out.setflags(write=False)
        _SCIPY[key] = (out, area)
    return _SCIPY[key]


def named_masks():
    """(name, mask u8 {0,1}) pairs; every mask small enough for a test of a few milliseconds."""
    out = []
    out.append(("empty", _canvas(9, 11)))
    out.append(("full", _canvas(9, 11) + 1))
    for name, (y, x) in (("corner-tl", (0, 0)), ("corner-tr", (0, 10)), ("corner-bl", (8, 0)), ("corner-br", (8, 10))):
        m = _canvas(9, 11)
        m[y, x] = 1
        out.append((name, m))
    ring = _canvas(12, 13)
    ring[2:9, 3:10] = 1
    ring[4:7, 5:8] = 0
    out.append(("ring", ring))
    isl = ring.copy()
    isl[5, 6] = 1
    out.append(("ring+island", isl))
    d = _canvas(9, 9)                      # a diamond outline: its interior is closed by diagonal steps only
    for k in range(4):
        d[4 - k, 1 + k] = d[4 + k, 1 + k] = d[4 - k, 7 - k] = d[4 + k, 7 - k] = 1
    d[1, 4] = d[7, 4] = 1
    out.append(("diamond", d))
    sq = _canvas(10, 10)
    sq[1:4, 1:4] = 1
    sq[4:8, 4:8] = 1
    out.append(("corner-touch", sq))
    cb = (np.indices((10, 11)).sum(0) % 2).astype(np.uint8)
    out.append(("checkerboard", cb))
    top = _canvas(21, 21)                  # what a spiral walker that never turns leaves: the top row
    top[0, :] = 1
    out.append(("top-row", top))
    out.append(("spiral", spiral(21)))
    comb = _canvas(10, 15)                 # teeth up to the top border: the pockets between them are open, not holes
    comb[8, 1:14] = 1
    comb[0:8, 1:14:2] = 1
    out.append(("comb", comb))
    spk = _canvas(14, 16)
    for y, x in ((0, 3), (2, 9), (5, 14), (11, 1), (13, 15)):
        spk[y, x] = 1
    spk[6:10, 5:9] = 1
    out.append(("specks+blob", spk))
    tie = _canvas(12, 20)                  # two 3x4 rectangles (equal keys), a smaller square, a speck
    tie[1:4, 1:5] = 1
    tie[7:10, 12:16] = 1
    tie[6:8, 2:4] = 1
    tie[0, 18] = 1
    out.append(("key-tie", tie))
    tie2 = _canvas(12, 20)                 # equal keys from different shapes: an L (three pixels) and a 2-pixel-wide step
    tie2[1, 1] = tie2[2, 1] = tie2[2, 2] = 1            # key 1
    tie2[6, 10] = tie2[6, 11] = tie2[7, 11] = 1         # key 1
    tie2[9:11, 3:5] = 1                                 # key 2
    out.append(("key-tie-2", tie2))
    rs = np.random.RandomState(77)
    for (h, w) in ((17, 23), (32, 48), (64, 64)):
        for dens in (0.3, 0.5, 0.6):
            out.append((f"random-{h}x{w}-{dens}", (rs.rand(h, w) < dens).astype(np.uint8)))
    return out


def sequence(seed, n, H, W):
    """A synthetic video for the guided-VFT pass: BGR u8 frames [n,H,W,3] with a dark, pulsating glottis-like gap (two lobes and a
    bright island), specks, and boxes as a detector would return them -- among them a run of ``None``, a negative coordinate
    (Python slice semantics), a box that leaves the frame, a box with at most 10 pixels and an empty one."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    frames = np.empty((n, H, W, 3), np.uint8)
    boxes = []
    cy, cx = H // 2, W // 2
    for i in range(n):
        base = 150 + 40 * np.sin(xx / 7.0 + i / 5.0) + rs.randint(-12, 13, (H, W))
        open_ = 0.35 + 0.3 * np.sin(i / 2.5)
        gap = (((yy - cy) / (H / 3.5)) ** 2 + ((xx - cx + 3) / (W * 0.09 * (0.4 + open_))) ** 2 < 1)
        gap |= (((yy - cy + 4) / (H / 6.0)) ** 2 + ((xx - cx - 6) / (W * 0.05)) ** 2 < 1)
        base[gap] = 25 + rs.randint(0, 20, int(gap.sum()))
        base[cy - 1:cy + 1, cx - 3:cx - 1] = 210                       # an island inside the gap
        dark = rs.rand(H, W) < 0.01
        base[dark] = 10
        g = np.clip(base, 0, 255)
        frames[i, ..., 0] = np.clip(g - 9, 0, 255)
        frames[i, ..., 1] = g
        frames[i, ..., 2] = np.clip(g + 7, 0, 255)
        j = rs.randint(-2, 3, 4)
        boxes.append((cx - W // 4 + j[0], cy - H // 3 + j[1], cx + W // 4 + j[2], cy + H // 3 + j[3]))
    for i in range(5, min(9, n)):
        boxes[i] = None
    if n > 10:
        boxes[10] = (-W + 4, -H + 3, -2, -1)          # counted from the far edge
    if n > 12:
        boxes[12] = (W // 2, H // 2, W + 30, H + 9)   # leaves the frame
    if n > 14:
        boxes[14] = (cx, cy, cx + 3, cy + 3)          # 9 pixels: n <= 10
    if n > 15:
        boxes[15] = (cx + 5, cy, cx + 5, cy + 9)      # empty
    if n > 17:
        boxes[17] = (-300, -300, 400, 400)            # larger than the frame
    return frames, boxes


def scipy_blobs(mask, n):
    """The blob filter stated with scipy.ndimage: -> (mask u8 {0,255}, area)."""
    from scipy import ndimage

    m = np.asarray(mask) > 0
    H, W = m.shape
    filled = ndimage.binary_fill_holes(m, structure=ndimage.generate_binary_structure(2, 1))
    lab, k = ndimage.label(filled, structure=np.ones((3, 3), int))
    if k == 0:
        return np.zeros((H, W), np.uint8), 0
    P = np.pad(lab, 1)
    win = np.stack([P[:-1, :-1], P[:-1, 1:], P[1:, :-1], P[1:, 1:]])
    cnt = (win > 0).sum(0)
    who = win.max(0)
    key = np.zeros(k + 1, np.int64)
    np.add.at(key, who[cnt == 4], 2)
    np.add.at(key, who[cnt == 3], 1)
    first = np.full(k + 1, H * W, np.int64)
    flat = lab.ravel()
    np.minimum.at(first, flat, np.arange(H * W))
    order = sorted(range(1, k + 1), key=lambda l: (key[l], first[l]), reverse=True)[:n]      # ties: the later first pixel wins
    out = np.isin(lab, order)
    return (out * 255).astype(np.uint8), int(out.sum())


_CONTOURS = {}


def contour_blobs(mask, n):
    """The blob filter as the reference's ``_nblobs`` composes it, over the cv2 stand-ins of tests/golden/gen_golden_vft.py:
    external contours by border following, sorted by the shoelace area (stable, largest first), the first n filled as polygons.
    -> (mask u8 {0,255}, area).  Pure Python: for sides up to 64."""
    import importlib.util
    import os
    import sys

    if "module" not in _CONTOURS:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen_golden_vft.py")
        spec = importlib.util.spec_from_file_location("gen_golden_vft", path)
        _CONTOURS["module"] = importlib.util.module_from_spec(spec)
        keep = list(sys.path)                                  # the generator prepends its own directories: not for the suite
        spec.loader.exec_module(_CONTOURS["module"])
        sys.path[:] = keep
    G = _CONTOURS["module"]
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    H, W = m.shape
    key = (m.tobytes(), m.shape)
    if key not in _CONTOURS:
        _CONTOURS[key] = sorted(G.find_external(m), key=G.contour_area, reverse=True)       # the order does not depend on n
    out = np.zeros((H, W), np.uint8)
    for c in _CONTOURS[key][:n]:
        out[G.polygon_fill([tuple(v) for v in c.reshape(-1, 2)], H, W)] = 255
    return out, int((out > 0).sum())


def otsu_numpy(hist):
    """Rule 8 in float64, one operation per statement."""
    h = np.asarray(hist, np.float64)
    n = h.sum()
    eps = np.float64(np.finfo(np.float32).eps)
    scale = np.float64(1.0) / n
    mu = np.float64(0.0)
    for i in range(256):
        mu = mu + np.float64(i) * h[i]
    mu = mu * scale
    mu1 = q1 = max_sigma = np.float64(0.0)
    best = 0
    for i in range(256):
        p = h[i] * scale
        mu1 = mu1 * q1
        q1 = q1 + p
        q2 = np.float64(1.0) - q1
        if min(q1, q2) < eps or max(q1, q2) > np.float64(1.0) - eps:
            continue
        mu1 = (mu1 + np.float64(i) * p) / q1
        mu2 = (mu - q1 * mu1) / q2
        d = mu1 - mu2
        sigma = q1 * q2 * d * d
        if sigma > max_sigma:
            max_sigma, best = sigma, i
    return best


def golden():
    """tests/golden/vft_guided.npz (tests/golden/gen_golden_vft.py: the reference's own tracker) as name -> dict with frames (BGR),
    boxes (tuples or None), init, seed (the threshold after initialize), thresh / area / masks of the processed frames, feats."""
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vft_guided.npz"))
    init, no_box = int(z["init"]), int(z["no_box"])
    out = {}
    for name in ("a", "b", "c"):
        frames = z[f"{name}_frames"]
        n, H, W = frames.shape[:3]
        boxes = [None if r[0] == no_box else tuple(int(v) for v in r) for r in z[f"{name}_boxes"]]
        th = z[f"{name}_thresh"]
        masks = np.unpackbits(z[f"{name}_masks"], axis=1)[:, :H * W].reshape(n - init, H, W) * 255
        feats = {k: (None if np.isnan(v) else float(v)) for k, v in zip(z[f"{name}_feat_keys"].tolist(), z[f"{name}_feat_vals"])}
        out[name] = dict(frames=frames, boxes=boxes, init=init, seed=float(th[0]), thresh=th[1:], area=z[f"{name}_area"],
                         masks=masks.astype(np.uint8), feats=feats)
    return out


class ScriptedDetector:
    """``reset`` / ``detect`` of a TemporalDetector, replaying boxes."""
    model = None

    def __init__(self, boxes):
        self.boxes, self.i = list(boxes), 0

    def reset(self):
        self.i = 0

    def detect(self, frame):
        b = self.boxes[self.i]
        self.i += 1
        return b
