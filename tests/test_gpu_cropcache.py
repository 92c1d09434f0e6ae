"""-m gpu: `cropcache.build` on the device against its host twin on the synthetic pairs of tests/cropcache_cases.py, both ROI modes:
the trees are identical byte for byte and meta.json is the same; k_label_bbox against its twin on labels whose object touches each
border, is one pixel, or is absent; the tiles-only entry against og_crop_tile_host inside guard zones."""
import numpy as np
import pytest
import torch

import buffer_guard as G
import cropcache_cases as CC
from openglottal_amd import cropcache
from openglottal_amd import png as P
from openglottal_amd._lib import check, lib

pytestmark = pytest.mark.gpu

SIZE = 32


@pytest.mark.parametrize("roi,padding", [("gt", 8), ("yolo", 8), ("yolo", 0)])
def test_device_cache_equals_the_host_twins(tmp_path, roi, padding):
    names, ips, lps = CC.write(str(tmp_path / "data"))
    res = {}
    for where in ("host", "device"):
        det = CC.Rows() if roi == "yolo" else None
        res[where] = cropcache.build(ips, lps, str(tmp_path / where), "train", roi=roi, detector=det, crop_size=SIZE, padding=padding,
                                     label_suffix="_seg", decode=where, encode=where)
    assert res["device"] == res["host"] and res["host"]["n"] >= 4
    a, b = CC.tree(str(tmp_path / "host")), CC.tree(str(tmp_path / "device"))
    assert a == b and len(a) == 2 * res["host"]["n"] + 1
    # mixed: device decode with host encode, and the other way round, give the same files
    det = CC.Rows() if roi == "yolo" else None
    cropcache.build(ips, lps, str(tmp_path / "mixed"), "train", roi=roi, detector=det, crop_size=SIZE, padding=padding, label_suffix="_seg",
                    decode="device", encode="host")
    det = CC.Rows() if roi == "yolo" else None
    cropcache.build(ips, lps, str(tmp_path / "mixed2"), "train", roi=roi, detector=det, crop_size=SIZE, padding=padding, label_suffix="_seg",
                    decode="host", encode="device")
    assert CC.tree(str(tmp_path / "mixed")) == a == CC.tree(str(tmp_path / "mixed2"))


def labels():
    H, W = 37, 53
    out = np.zeros((8, H, W), np.uint8)
    out[0, 0, 20] = 255                                                       # touches the top
    out[1, H - 1, 7] = 1                                                      # the bottom
    out[2, 11:15, 0] = 200                                                    # the left
    out[3, 30, W - 1] = 3                                                     # the right
    out[4, 17, 29] = 255                                                      # one pixel
    out[6] = 255                                                              # every pixel; 5: none
    out[7, 3:9, 40:50] = 9
    out[7, 20, 2] = 1
    return out


def test_k_label_bbox_against_its_twin():
    lab = labels()
    B, H, W = lab.shape
    e = P.PngEncoder()
    got = e.label_bbox_dev(torch.from_numpy(lab).cuda(), B, H, W).cpu().numpy()
    want = np.array([cropcache.label_bbox_host(l) for l in lab], np.int32)
    assert np.array_equal(got, want)
    assert want.tolist() == [[20, 0, 21, 1], [7, H - 1, 8, H], [0, 11, 1, 15], [W - 1, 30, W, 31], [29, 17, 30, 18], [0, 0, 0, 0], [0, 0, W, H],
                             [2, 3, 50, 21]]
    for l, b in zip(lab, want):                                               # numpy's word on it
        if l.max():
            ys, xs = np.where(l > 0)
            assert b.tolist() == [xs.min(), ys.min(), xs.max() + 1, ys.max() + 1]


def test_label_bbox_and_crop_tiles_hold_their_extents():
    lab = labels()
    B, H, W = lab.shape
    e = P.PngEncoder()
    sync = lambda: check(lib().og_pnge_sync(e._h), "og_pnge_sync")   # noqa: E731
    out = G.run_guarded("og_pnge_label_bbox_u8_dev", "8 labels", lambda p: lib().og_pnge_label_bbox_u8_dev(e._h, p["labels"], B, H, W, p["boxes"]),
                        {"labels": lab}, {"boxes": 16 * B}, "device", sync=sync)
    assert np.array_equal(out["boxes"].view(np.int32).reshape(B, 4), [cropcache.label_bbox_host(l) for l in lab])
    frames = np.random.default_rng(3).integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    boxes = np.array([[2, 3, 50, 21], [0, 0, W, H], [5, 5, 5, 9]], np.int32)   # the last one is not usable: a zero tile
    for ch, src in ((3, frames), (1, np.ascontiguousarray(lab[[7, 6, 0]]))):
        out = G.run_guarded("og_pnge_crop_tiles_u8_dev", f"ch={ch}",
                            lambda p: lib().og_pnge_crop_tiles_u8_dev(e._h, p["frames"], 3, H, W, ch, p["boxes"], SIZE, p["tiles"]),
                            {"frames": src, "boxes": boxes}, {"tiles": 3 * SIZE * SIZE}, "device", sync=sync)
        tiles = out["tiles"].reshape(3, SIZE, SIZE)
        assert np.array_equal(tiles[0], cropcache.crop_tile_host(src[0], boxes[0], SIZE)) and tiles[0].any()
        assert np.array_equal(tiles[1], cropcache.crop_tile_host(src[1], boxes[1], SIZE)) and not tiles[2].any()
    print(G.report())
