"""Helper module of the overlay tests (tests/test_overlay_*.py, tests/test_gpu_overlay*.py): an independent numpy / scipy statement
of the four drawing rules of include/openglottal_hip_overlay.h (source, fill, outline, rectangle), the box cases, and the frames
the GPU tests draw on.  Nothing here calls the library."""
import numpy as np

STYLES = ("none", "contour", "fill")
ABSENT = "absent"                          # a call without boxes at all (the unet-only pipeline), as overlay.overlay_host takes it


def outside_background(mask):
    """bool [H,W]: the union of the 4-connected background components that touch the frame's edge (scipy.ndimage.label)."""
    from scipy import ndimage

    bg = np.asarray(mask) == 0
    lab, _ = ndimage.label(bg, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    edge = np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]])
    return np.isin(lab, np.setdiff1d(np.unique(edge), [0])) & bg


def outline(mask):
    """bool [H,W]: set, and on the frame's edge or 4-adjacent to the outside background."""
    m = np.asarray(mask) != 0
    out = outside_background(mask)
    near = np.zeros_like(m)
    near[0, :] = near[-1, :] = near[:, 0] = near[:, -1] = True
    near[1:, :] |= out[:-1, :]
    near[:-1, :] |= out[1:, :]
    near[:, 1:] |= out[:, :-1]
    near[:, :-1] |= out[:, 1:]
    return m & near


def outline_filled(mask):
    """The issue's second statement: a pixel of the HOLE-FILLED mask with a 4-neighbour off the hole-filled mask or off the frame."""
    filled = ~outside_background(mask)
    p = np.pad(filled, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return filled & ~inner


def rectangle(H, W, box):
    """bool [H,W]: the one-pixel rectangle with both corners inclusive, clipped to the frame, by plain slicing."""
    x1, y1, x2, y2 = (int(v) for v in box)
    r = np.zeros((H, W), bool)
    xa, xb = max(x1, 0), min(x2, W - 1)
    ya, yb = max(y1, 0), min(y2, H - 1)
    for y in (y1, y2):
        if 0 <= y < H and xa <= xb:
            r[y, xa:xb + 1] = True
    for x in (x1, x2):
        if 0 <= x < W and ya <= yb:
            r[ya:yb + 1, x] = True
    return r


def overlay(frame, mask, box, style):
    """One frame by the rules, in order.  ``box``: a normalised ``(x1, y1, x2, y2)`` row (x1 < 0: None: nothing is drawn) or ABSENT."""
    f = np.asarray(frame)
    out = np.repeat(f[:, :, None], 3, axis=2).copy() if f.ndim == 2 else f.copy()
    H, W = f.shape[:2]
    absent = isinstance(box, str)
    if not absent and box[0] < 0:
        return out
    if mask is not None and style != "none":
        m = np.asarray(mask) != 0
        if style == "fill":
            g = out[:, :, 1].astype(np.int32)
            out[:, :, 1] = np.where(m, np.minimum(255, g + 102), g).astype(np.uint8)
        out[outline(mask)] = (0, 255, 0)
    if not absent:
        out[rectangle(H, W, box)] = (0, 220, 255)
    return out


def box_cases(H, W):
    """(name, normalised box row) pairs: None, one pixel, the far corner at x2 == W / y2 == H, row 0, column 0, an inner box."""
    return [
        ("none", (-1, -1, -1, -1)),
        ("one-pixel", (W // 2, H // 3, W // 2, H // 3)),
        ("far-corner", (W // 4, H // 4, W, H)),
        ("row-0", (2, 0, W - 3, H // 2)),
        ("column-0", (0, 3, W // 2, H - 2)),
        ("inner", (3, 5, W - 4, H - 6)),
    ]


def frames_for(n, H, W, channels, seed):
    rs = np.random.RandomState(seed)
    shape = (n, H, W, 3) if channels == 3 else (n, H, W)
    f = rs.randint(0, 256, shape).astype(np.uint8)
    f[0] = 153 if n else 0                 # G + 102 == 255 exactly
    if n > 1:
        f[1] = 154                         # the first value that saturates
    return f


def cut(mask, H, W):
    """A mask cut or zero-padded to [H,W], values {0, 255}."""
    out = np.zeros((H, W), np.uint8)
    h, w = min(H, mask.shape[0]), min(W, mask.shape[1])
    out[:h, :w] = (np.asarray(mask)[:h, :w] != 0) * 255
    return out
