"""``YOLOGuidedVFT`` (`openglottal/models/tracker.py:117-232`) on the device: the per-frame surface `scripts/infer.py` uses.

The reference's tracker keeps an EMA motion map (``lmap``) that it updates every frame and never reads, so no output depends on
``alpha`` or ``gaussian_ksize``; they are accepted for signature compatibility and have no effect here either, and ``lmap`` stays
``None``.  What the mask depends on -- the box, the percentile inside it, the beta-smoothed threshold and the n-largest-blob filter --
runs in ``libopenglottal_hip.so`` (``classic.Classic``).  ``VocalFoldTracker`` (pipeline ``vft``) is not provided: its ROI comes from
thresholding a Gaussian-blurred f32 motion map, which cannot be pinned without OpenCV.
"""
from __future__ import annotations

import numpy as np

from ._lib import OpenGlottalHipError
from .classic import Classic


class YOLOGuidedVFT:
    def __init__(self, alpha: float = 0.98, beta: float = 0.7, glottal_percentile: int = 5, gaussian_ksize: int = 13,
                 max_glottal_components: int = 2) -> None:
        self.alpha = alpha            # no effect on any output (as in the reference)
        self.beta = beta
        self.pct = glottal_percentile
        self.gk = (gaussian_ksize, gaussian_ksize)   # no effect on any output (as in the reference)
        self.n_comp = max_glottal_components
        self.prev = None
        self.lmap = None
        self._engine = Classic(beta, glottal_percentile, max_glottal_components, tiled="auto")
        self._seeded = False

    @property
    def thresh(self):
        return self._engine.thresh if self._seeded else None

    @thresh.setter
    def thresh(self, value) -> None:
        self._engine.thresh = float(value)
        self._seeded = True

    def initialize(self, frames, bbox=None) -> None:
        """Seed the intensity threshold from the last of ``frames`` (gray or BGR u8) inside ``bbox`` (whole frame when ``None``)."""
        self._engine.init(list(frames), bbox)
        self._seeded = True

    def process_frame(self, frame: np.ndarray, bbox) -> np.ndarray:
        """Gray (or BGR) u8 full-resolution frame and the detector's box for it (``None``: empty mask) -> u8 mask, 255 = glottis."""
        if not self._seeded:
            raise OpenGlottalHipError("YOLOGuidedVFT.process_frame before initialize")
        mask, _ = self._engine.guided_vft(np.asarray(frame)[None], [bbox])
        return mask[0]

    def process_frames(self, frames, boxes, want_mask: bool = True):
        """``process_frame`` over many frames in one streamed device pass: ``(masks | None, areas)``."""
        if not self._seeded:
            raise OpenGlottalHipError("YOLOGuidedVFT.process_frames before initialize")
        return self._engine.guided_vft(frames, boxes, want_mask=want_mask)
