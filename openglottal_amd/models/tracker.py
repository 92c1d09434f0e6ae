from ..tracker import YOLOGuidedVFT  # noqa: F401
