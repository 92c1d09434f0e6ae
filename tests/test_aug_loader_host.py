"""`augment.CropCacheLoader` with decode="host" and the twin, on a cache `cropcache.build(..., decode="host", encode="host")` made from
tests/cropcache_cases.py: a sample's tensors depend on (seed, epoch, sample) only, an epoch yields every sample once, and a cache whose
meta.json disagrees with its files is refused.  No GPU."""
import json
import os

import numpy as np
import pytest

import aug_cases as AC
import cropcache_cases as CC
from openglottal_amd import augment as A
from openglottal_amd import cropcache
from openglottal_amd._lib import OpenGlottalHipError

SIZE = 32


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("augcache")
    _, ips, lps = CC.write(str(tmp / "data"))
    res = cropcache.build(ips, lps, str(tmp / "cache"), "train", roi="gt", crop_size=SIZE, padding=8, label_suffix="_seg", decode="host",
                          encode="host")
    assert res["n"] == 5
    return str(tmp / "cache"), res["n"]


def by_sample(loader, epoch):
    """{sample: (img, msk)} of one epoch, and how often each sample came"""
    loader.set_epoch(epoch)
    order, out, at, shapes = loader.order(epoch), {}, 0, []
    for imgs, msks in loader:
        assert imgs.dtype == msks.dtype == np.float32 and imgs.shape == msks.shape and imgs.shape[1:] == (1, SIZE, SIZE)
        shapes.append(imgs.shape[0])
        for k in range(imgs.shape[0]):
            assert order[at] not in out
            out[order[at]] = (imgs[k].copy(), msks[k].copy())
            at += 1
    assert loader.epoch == epoch + 1
    return out, shapes


def test_the_tiles_are_the_caches(cache):
    path, n = cache
    l = A.CropCacheLoader(path, "train", batch=2, decode="host")
    assert (l.n, l.crop_size, len(l)) == (n, SIZE, 3) and l.images.shape == l.masks.shape == (n, SIZE, SIZE) and l.images.dtype == np.uint8
    for k in range(n):
        assert np.array_equal(l.images[k], CC.gray_of(os.path.join(path, "train", "images", f"{k:06d}.png")))
        assert np.array_equal(l.masks[k], CC.gray_of(os.path.join(path, "train", "masks", f"{k:06d}.png")))


def test_a_samples_tensors_depend_on_seed_epoch_and_sample_only(cache):
    path, n = cache
    runs = {}
    for batch in (1, 3, n):
        l = A.CropCacheLoader(path, "train", batch=batch, seed=7, decode="host")
        for epoch in (0, 1):
            got, shapes = by_sample(l, epoch)
            assert sorted(got) == list(range(n))                              # epoch coverage: every sample once
            assert shapes == [batch] * (n // batch) + ([n % batch] if n % batch else []) and len(shapes) == len(l)
            runs[(batch, epoch)] = got
    for epoch in (0, 1):
        for batch in (3, n):
            for s in range(n):
                for a, b in zip(runs[(1, epoch)][s], runs[(batch, epoch)][s]):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (epoch, batch, s)
    assert any(not np.array_equal(runs[(1, 0)][s][0], runs[(1, 1)][s][0]) for s in range(n))            # another epoch: other draws
    other, _ = by_sample(A.CropCacheLoader(path, "train", batch=n, seed=8, decode="host"), 0)
    assert any(not np.array_equal(runs[(1, 0)][s][0], other[s][0]) for s in range(n))                   # another seed too
    l = A.CropCacheLoader(path, "train", batch=2, seed=7, decode="host")
    assert l.order(0) != l.order(1) or l.order(1) != l.order(2)
    rec = A.sample_record(7, 0, 3, SIZE)                                      # and it is the twin on the record of (seed, epoch, sample)
    oi, om = A.augment_host(l.images, l.masks, [3], [rec])
    assert np.array_equal(oi[0], runs[(1, 0)][3][0]) and np.array_equal(om[0], runs[(1, 0)][3][1])
    assert set(np.unique(om)) <= {0.0, 1.0} and oi.min() >= 0 and oi.max() <= 1


def test_without_augmentation_and_without_shuffling(cache):
    path, n = cache
    l = A.CropCacheLoader(path, "train", batch=2, augment=False, shuffle=False, decode="host")
    assert l.order(0) == l.order(5) == list(range(n))
    got, _ = by_sample(l, 0)
    for s in range(n):
        assert np.array_equal(got[s][0][0], l.images[s].astype(np.float32) / np.float32(255.0)) and np.array_equal(got[s][1][0], (l.masks[s] > 0).astype(np.float32))


def test_arrays_in_place_of_a_cache_directory():
    im, mk = AC.tiles(SIZE)
    l = A.CropCacheLoader((im, mk), batch=3, seed=1, decode="host")
    got, shapes = by_sample(l, 0)
    assert shapes == [3, 1] and sorted(got) == [0, 1, 2, 3]
    oi, _ = A.augment_host(im, mk, [2], [A.sample_record(1, 0, 2, SIZE)])
    assert np.array_equal(got[2][0], oi[0])
    for bad in ((im, mk[:2]), (im[:, :, :30], mk[:, :, :30]), (im[0], mk[0])):
        with pytest.raises(OpenGlottalHipError):
            A.CropCacheLoader(bad, decode="host")
    with pytest.raises(OpenGlottalHipError):
        A.CropCacheLoader((im, mk), decode="gpu")
    with pytest.raises(OpenGlottalHipError):
        A.CropCacheLoader((im, mk), batch=0, decode="host")


def test_a_cache_whose_meta_disagrees_with_its_files_is_refused(tmp_path):
    im, mk = AC.tiles(SIZE)
    for name, kw, why in (("n", {"n": 5}, "n = 5"), ("size", {"crop_size": 64}, "crop_size = 64")):
        AC.write_cache(str(tmp_path / name), "train", im, mk, **kw)
        with pytest.raises(OpenGlottalHipError, match=why):
            A.CropCacheLoader(str(tmp_path / name), "train", decode="host")
    AC.write_cache(str(tmp_path / "ok"), "train", im, mk)
    assert A.CropCacheLoader(str(tmp_path / "ok"), "train", decode="host").n == 4
    with pytest.raises(OpenGlottalHipError, match="meta.json"):
        A.CropCacheLoader(str(tmp_path / "ok"), "val", decode="host")         # no such split
    os.remove(tmp_path / "ok" / "train" / "masks" / "000003.png")            # a mask short
    with pytest.raises(OpenGlottalHipError, match="masks"):
        A.CropCacheLoader(str(tmp_path / "ok"), "train", decode="host")
    with open(tmp_path / "ok" / "train" / "meta.json", "w") as fh:
        fh.write(json.dumps({"crop_size": SIZE}))                             # no n
    with pytest.raises(OpenGlottalHipError, match="meta.json"):
        A.CropCacheLoader(str(tmp_path / "ok"), "train", decode="host")
