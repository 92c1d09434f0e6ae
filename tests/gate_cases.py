"""Helper module (like tests/sweep_cases.py) of the tests of include/openglottal_hip_gate.h: which frames a test keeps, and the boxes
that say so.  numpy only."""
import numpy as np

SELECT_B = (0, 1, 255, 256, 257, 513)     # empty, one frame, one short of / exactly / one past k_gate_select's block, three blocks
NO_BOX = (-1, -1, -1, -1)                 # utils.normalize_box(None, ...)


def patterns(B, seed=0):
    """name -> bool [B]: which frames are kept."""
    rs = np.random.RandomState(1000 + B + seed)
    idx = np.arange(B)
    out = {"none": np.zeros(B, bool), "all": np.ones(B, bool), "alternating": idx % 2 == 0, "first only": idx == 0, "last only": idx == B - 1,
           "random": rs.rand(B) < 0.5}
    return out


def boxes_for(kept, W=160, H=96, seed=0):
    """int32 [B,4]: NO_BOX for a frame that is not kept; for a kept one a box with x1 = 0 (the boundary of the rule) on every other
    kept frame, the empty slice (0,0,0,0) on every fifth, and a box inside the frame otherwise."""
    kept = np.asarray(kept, bool)
    rs = np.random.RandomState(7 + len(kept) + seed)
    b = np.tile(np.array(NO_BOX, np.int32), (len(kept), 1))
    for r, i in enumerate(np.flatnonzero(kept)):
        x1 = 0 if r % 2 == 0 else int(rs.randint(1, W // 2))
        y1 = int(rs.randint(0, H // 2))
        b[i] = (0, 0, 0, 0) if r % 5 == 4 else (x1, y1, int(rs.randint(W // 2, W + 1)), int(rs.randint(H // 2, H + 1)))
    return b


def keep_of(boxes):
    """The rule in numpy: ascending indices of the frames whose box has x1 >= 0."""
    return np.flatnonzero(np.asarray(boxes).reshape(-1, 4)[:, 0] >= 0).astype(np.int32)
