#!/usr/bin/env python3
"""The 512 x 512 BGR stream alone (for `rocprofv3 --kernel-trace --stats -- python tools/bench_resized_trace.py`): 512 frames
through UNet.segment_resized, so that the stats show the two resize kernels next to the chain's."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_resized import model, video  # noqa: E402

m = model()
v = video(512, 512, 512)
_, area = m.segment_resized(v, want_mask=False)
print("frames", len(area), "mean area", float(area.mean()))
