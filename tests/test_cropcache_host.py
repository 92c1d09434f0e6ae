"""`cropcache.build` with host decode and host encode (the twin the device is held to) on the synthetic pairs of
tests/cropcache_cases.py: the files, their numbering and meta.json, the hash recomputed here, every tile against og_crop_tile_host of a
box computed here in numpy, and the skip rules of both ROI modes.  The detector is replaced by given best rows.  No GPU."""
import hashlib
import json
import os

import numpy as np
import pytest

import cropcache_cases as CC
from openglottal_amd import cli, cropcache
from openglottal_amd import png as P

SIZE = 32


def build(tmp_path, roi, padding, **kw):
    names, ips, lps = CC.write(str(tmp_path / "data"))
    det = CC.Rows() if roi == "yolo" else None
    res = cropcache.build(ips, lps, str(tmp_path / "cache"), "train", roi=roi, detector=det, crop_size=SIZE, padding=padding,
                          label_suffix="_seg", decode="host", encode="host", **kw)
    return names, res, det


@pytest.mark.parametrize("roi,padding", [("gt", 8), ("gt", 0), ("yolo", 8), ("yolo", 0)])
def test_files_numbering_meta_and_tiles(tmp_path, roi, padding):
    names, res, det = build(tmp_path, roi, padding)
    want = CC.expected_boxes(roi, padding)
    if roi == "yolo" and padding == 0:
        assert want.pop(CC.SLIVER)[3] - 30 == 1                              # one pixel high: its content rounds to no row at all
    kept = sorted(want)
    assert res["kept"] == kept and res["boxes"] == [want[i] for i in kept] and res["n"] == len(kept)
    base = tmp_path / "cache" / "train"
    files = [f"{k:06d}.png" for k in range(len(kept))]
    assert sorted(os.listdir(base)) == ["images", "masks", "meta.json"]
    assert sorted(os.listdir(base / "images")) == files and sorted(os.listdir(base / "masks")) == files
    meta = json.loads((base / "meta.json").read_text())
    digest = hashlib.sha256(",".join(sorted(names)).encode()).hexdigest()[:16]
    assert meta == {"n": len(kept), "crop_size": SIZE, "label_suffix": "_seg", "source_hash": digest, "roi_mode": roi} == res["meta"]
    assert list(meta) == ["n", "crop_size", "label_suffix", "source_hash", "roi_mode"]
    assert cropcache.cache_valid(str(tmp_path / "cache"), "train", names, SIZE, "_seg")
    assert not cropcache.cache_valid(str(tmp_path / "cache"), "train", names[:-1], SIZE, "_seg")
    assert not cropcache.cache_valid(str(tmp_path / "cache"), "train", names, SIZE, "")
    assert not cropcache.cache_valid(str(tmp_path / "cache"), "val", names, SIZE, "_seg")
    pairs = CC.pairs()
    for k, i in enumerate(kept):
        _, bgr, lab = pairs[i]
        tile, mask = CC.gray_of(str(base / "images" / files[k])), CC.gray_of(str(base / "masks" / files[k]))
        assert tile.shape == mask.shape == (SIZE, SIZE)
        assert np.array_equal(tile, cropcache.crop_tile_host(bgr, want[i], SIZE)), (roi, i)
        assert np.array_equal(mask, cropcache.crop_tile_host(lab, want[i], SIZE)), (roi, i)
        assert set(np.unique(mask)) <= {0, 1, 255} and mask.max() == lab[want[i][1]:want[i][3], want[i][0]:want[i][2]].max()
        assert open(base / "images" / files[k], "rb").read() == P.encode_host(tile)
    if det is not None:                                                       # the detector saw every frame once, run by run
        assert [c[:2] for c in det.calls] == [(2, (64, 96, 3)), (2, (80, 72, 3)), (1, (64, 96, 3)), (1, (80, 72, 3))]
        assert all(c[2] == 0.25 for c in det.calls)


def test_the_skip_rules():
    assert cropcache.gt_box((0, 0, 0, 0), 64, 96, 8) is None                  # an empty label
    assert cropcache.gt_box((5, 6, 6, 7), 64, 96, 8) == (0, 0, 14, 15)        # one pixel, padded and clipped
    assert cropcache.gt_box((90, 60, 96, 64), 64, 96, 8) == (82, 52, 96, 64)
    assert cropcache.yolo_box((1, 2, 3, 4, -1), 64, 96, 8) is None            # no detection
    assert cropcache.yolo_box((20.9, 10.9, 70.1, 50.9, 0.5), 64, 96, 8) == (12, 2, 78, 58)      # int() cuts, then the padding
    assert cropcache.yolo_box((3.2, 1.0, 95.5, 63.2, 0.5), 64, 96, 8) == (0, 0, 96, 64)
    assert not cropcache.usable(None, 32) and not cropcache.usable((5, 5, 5, 9), 32) and not cropcache.usable((3, 30, 70, 31), 32)
    assert cropcache.usable((3, 30, 70, 32), 32) and cropcache.usable((0, 0, 1, 1), 32)
    assert cropcache.label_bbox_host(np.zeros((4, 5), np.uint8)) == (0, 0, 0, 0)


def test_a_confidence_above_every_row_keeps_nothing_and_writes_no_meta(tmp_path):
    names, res, _ = build(tmp_path, "yolo", 8, conf=0.95)
    assert res == {"n": 0, "kept": [], "boxes": [], "meta": None} and not os.path.exists(tmp_path / "cache" / "train" / "meta.json")


def test_bad_arguments(tmp_path):
    names, ips, lps = CC.write(str(tmp_path / "data"))
    for kw in ({"roi": "box"}, {"roi": "yolo"}, {"decode": "gpu"}, {"crop_size": 0}, {"padding": -1}):
        with pytest.raises(cropcache.OpenGlottalHipError):
            cropcache.build(ips, lps, str(tmp_path / "c"), "train", **{"roi": "gt", "decode": "host", "encode": "host", **kw})
    with pytest.raises(cropcache.OpenGlottalHipError):
        cropcache.build(ips, lps[:-1], str(tmp_path / "c"), "train", roi="gt", decode="host", encode="host")
    with pytest.raises(cropcache.OpenGlottalHipError):                        # a label of another size than its image
        cropcache.build(ips[:1], lps[2:3], str(tmp_path / "c"), "train", roi="gt", decode="host", encode="host")
    assert not os.path.exists(tmp_path / "c")


def test_cli_crop_cache_on_the_host(tmp_path, capsys):
    names, ips, lps = CC.write(str(tmp_path / "data"))
    os.remove(lps[5])                                                         # a pair without a label: not built, still hashed
    argv = ["crop-cache", "--images", str(tmp_path / "data"), "--labels", str(tmp_path / "data"), "--out", str(tmp_path / "cache"), "--split",
            "val", "--roi", "gt", "--label-suffix", "_seg", "--crop-size", str(SIZE), "--host"]
    assert cli.main(argv) == 0
    assert "4 of 6 samples kept" in capsys.readouterr().out                   # six images, one without a label, one label empty
    assert cropcache.cache_valid(str(tmp_path / "cache"), "val", names, SIZE, "_seg")
    assert sorted(os.listdir(tmp_path / "cache" / "val" / "masks")) == [f"{k:06d}.png" for k in range(4)]
    assert cli.main(argv + ["--max-images", "2"]) == 0 and "2 of 2 samples kept" in capsys.readouterr().out
