"""CPU: the detector's ``"precision"`` option at the C-ABI (no device work: the handle is created, never finalized)."""
import os

from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OG_EINVAL = -1


def test_precision_option_accepts_0_and_2_and_refuses_1_and_3():
    h = lib().og_yolo_create(1)
    assert h
    try:
        assert lib().og_yolo_set_option(h, b"precision", 0) == 0
        assert lib().og_yolo_set_option(h, b"precision", 2) == 0
        assert lib().og_yolo_set_option(h, b"precision", 0) == 0
        for v in (1, 3, 4, -1):
            assert lib().og_yolo_set_option(h, b"precision", v) == OG_EINVAL, v
    finally:
        lib().og_yolo_destroy(h)


def test_header_and_integration_guide_document_the_option():
    hdr = open(os.path.join(ROOT, "include", "openglottal_hip.h")).read()
    i = hdr.index("int og_yolo_set_option(")
    doc = hdr[hdr.rindex("/*", 0, i):i]
    assert '"precision"' in doc and "OG_EINVAL" in doc and "OG_ERANGE" in doc and "f16" in doc
    guide = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "og_yolo_set_option" in guide and "--detector-precision" in guide


def test_python_wrapper_maps_the_precision_names():
    from openglottal_amd.yolo import PRECISIONS

    assert PRECISIONS == {"f32": 0, "f16": 2}
