"""openglottal_amd — MI355X-native glottal segmentation hot path.

Drop-in names of the reference package (`openglottal/__init__.py:5-20`) for the
per-frame segmentation path; everything heavy runs in ``libopenglottal_hip.so``.
"""

__version__ = "0.1.0"

from ._lib import OpenGlottalHipError  # noqa: F401
from .detector import TemporalDetector  # noqa: F401
from .features import (_kinematic_features, extract_features_unet, extract_features_unet_crop,  # noqa: F401
                       extract_features_yolo_guided_vft, extract_gaw_features)
from .sweep import Sweep, conf_sweep, hold_ablation, sweep_host  # noqa: F401
from .tracker import YOLOGuidedVFT  # noqa: F401
from .unet import UNet  # noqa: F401
from .utils import dice, iou, unet_segment_frame  # noqa: F401

__all__ = ["UNet", "TemporalDetector", "extract_features_unet", "extract_features_unet_crop", "extract_features_yolo_guided_vft",
           "YOLOGuidedVFT", "unet_segment_frame", "dice", "iou",
           "extract_gaw_features", "OpenGlottalHipError", "Sweep", "sweep_host", "hold_ablation", "conf_sweep"]
