"""The arithmetic of the YOLO-Crop+UNet video pipeline on the host (include/openglottal_hip_crops.h): og_crop_geometry_host,
og_crop_tile_host and og_crop_project_host run the very inline functions of csrc/og_kernels.hpp that k_crop_tiles / k_crop_project
call, so this module judges the kernels' arithmetic against geometry.py (the reference's letterbox / unletterbox as restated in
numpy) without a GPU.  The CLI's new pipeline choice is parsed here too."""
import numpy as np
import pytest

import crop_cases as K
from openglottal_amd import geometry
from openglottal_amd.utils import bgr_to_gray_numpy


@pytest.mark.parametrize("size", [32, 64, 256])
def test_geometry_equals_letterbox_with_info_for_every_crop_up_to_130(size):
    n_zero = 0
    for h in range(1, 131):
        for w in range(1, 131):
            rc, g = K.geometry_host(h, w, size)
            assert rc == 0
            s = size / max(h, w)
            nh, nw = int(round(h * s)), int(round(w * s))
            assert (g[2] == 0) == (nh == 0) and (g[3] == 0) == (nw == 0), (h, w, g)     # a 0 side exactly where Python rounds to 0
            if nh == 0 or nw == 0:
                n_zero += 1
                continue
            assert g == geometry.letterbox_with_info(np.zeros((h, w), np.uint8), size)[1:], (h, w, g)
            assert g == geometry.letterbox_geometry(h, w, size)
    assert (n_zero > 0) == (size < 256)      # 1 x 65 at 32, 1 x 129 at 64; nothing up to 130 at 256


def test_geometry_half_way_cases_round_to_even():
    """Python's round() is half to even; floor(x + 0.5) gives (7, 0, 17, 32), (6, 0, 19, 32) and (0, 7, 32, 17) here."""
    assert K.geometry_host(33, 64, 32) == (0, (8, 0, 16, 32))
    assert K.geometry_host(35, 64, 32) == (0, (7, 0, 18, 32))
    assert K.geometry_host(64, 33, 32) == (0, (0, 8, 32, 16))
    for h, w, want in ((33, 64, (8, 0, 16, 32)), (35, 64, (7, 0, 18, 32)), (64, 33, (0, 8, 32, 16))):
        assert geometry.letterbox_with_info(np.zeros((h, w), np.uint8), 32)[1:] == want
    assert K.geometry_host(1, 64, 32) == (0, (16, 0, 0, 32))      # round(0.5) = 0: reported, rc 0
    assert K.geometry_host(1, 63, 32) == (0, (15, 0, 1, 32))


def test_geometry_refuses_bad_arguments():
    from openglottal_amd._lib import lib

    g = np.zeros(4, np.int32)
    for h, w, size in ((0, 5, 32), (5, 0, 32), (5, 5, 0), (-3, 5, 32)):
        assert lib().og_crop_geometry_host(h, w, size, g.ctypes.data) == -1
    assert lib().og_crop_geometry_host(5, 5, 32, None) == -1


def _frames():
    rs = np.random.RandomState(3)
    bgr = rs.randint(0, 256, (K.H, K.W, 3), dtype=np.uint8)
    return bgr, bgr_to_gray_numpy(bgr)


def test_tile_equals_letterbox_of_the_crop_gray_and_bgr():
    bgr, gray = _frames()
    for box in K.USABLE:
        want, top, left, nh, nw = K.numpy_tile(gray, box, K.SIZE)
        assert nh >= 1 and nw >= 1
        assert K.geometry_host(box[3] - box[1], box[2] - box[0], K.SIZE)[1] == (top, left, nh, nw)
        assert np.array_equal(K.tile_host(gray, box, K.SIZE), want), box
        assert np.array_equal(K.tile_host(bgr, box, K.SIZE), want), box       # BGR2GRAY per tap == convert, then crop
    for size in (64, 256):      # upscale of every box
        for box in K.USABLE:
            assert np.array_equal(K.tile_host(bgr, box, size), K.numpy_tile(gray, box, size)[0]), (size, box)


def test_projection_equals_unletterbox_paste_and_sum():
    rs = np.random.RandomState(4)
    for i, box in enumerate(K.USABLE):
        geom = K.geometry_host(box[3] - box[1], box[2] - box[0], K.SIZE)[1]
        tm = (rs.randint(0, 2, (K.SIZE, K.SIZE)) * 255).astype(np.uint8)
        want_mask, want_area = K.numpy_project(tm, box, geom, K.H, K.W)
        mask, area = K.project_host(tm, box, K.H, K.W)
        assert np.array_equal(mask, want_mask) and area == want_area == int((mask > 0).sum()), box
        assert K.project_host(tm, box, K.H, K.W, want_mask=False) == (None, want_area)
        assert 0 < area < (box[2] - box[0]) * (box[3] - box[1]) or (box[2] - box[0]) * (box[3] - box[1]) < 8, (box, area)


def test_unusable_boxes_give_area_zero_and_zero_masks():
    bgr, gray = _frames()
    tm = np.full((K.SIZE, K.SIZE), 255, np.uint8)
    for box in K.UNUSABLE:
        assert not K.tile_host(gray, box, K.SIZE).any() and not K.tile_host(bgr, box, K.SIZE).any(), box
        mask, area = K.project_host(tm, box, K.H, K.W)
        assert area == 0 and not mask.any(), box
    # the sliver is usable at a tile size where its short side rounds to 1
    x1, y1, x2, y2 = K.SLIVER
    assert K.geometry_host(y2 - y1, x2 - x1, 64)[1][3] == 1
    assert np.array_equal(K.tile_host(gray, K.SLIVER, 64), K.numpy_tile(gray, K.SLIVER, 64)[0])


def test_cli_crop_pipeline_needs_crop_weights_and_old_pipelines_parse_as_before(capsys, monkeypatch):
    from openglottal_amd import cli

    with pytest.raises(SystemExit) as e:
        cli.main(["run", "video.npy", "--pipeline", "yolo-crop+unet", "--yolo-weights", "y.npz", "--unet-weights", "u.pt"])
    assert e.value.code == 2 and "--crop-weights is required" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(["run", "video.npy", "--pipeline", "unet"])          # as before: argparse asks for --unet-weights
    assert e.value.code == 2 and "--unet-weights" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(["run", "video.npy", "--pipeline", "unet", "--unet-weights", "u.pt"])
    assert e.value.code == 2 and "--yolo-weights is required for --pipeline unet" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(["run", "video.npy", "--pipeline", "no-such", "--unet-weights", "u.pt"])
    assert e.value.code == 2
    # the two old choices get past the parser: the first thing after it is the model on the device
    import openglottal_amd

    seen = []

    class Stop(Exception):
        pass

    def fake_unet(*a, **k):
        seen.append(a)
        raise Stop

    monkeypatch.setattr(openglottal_amd, "UNet", fake_unet)
    for argv in (["--pipeline", "unet-only", "--unet-weights", "u.pt"], ["--pipeline", "unet", "--unet-weights", "u.pt", "--yolo-weights", "y.npz"],
                 ["--unet-weights", "u.pt"], ["--pipeline", "yolo-crop+unet", "--crop-weights", "c.pt", "--yolo-weights", "y.npz"]):
        with pytest.raises(Stop):
            cli.main(["run", "video.npy"] + argv)
    assert len(seen) == 4
