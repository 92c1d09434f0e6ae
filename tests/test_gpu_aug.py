"""-m gpu: the device augmentation (og_aug_batch_u8_dev: k_aug_rotate, k_aug_scale, k_aug_blur, k_aug_contrast, k_aug_plain) against
its host twin, bit for bit, on the case list of tests/aug_cases.py; the loader's (seed, epoch, sample) invariance; the device loader
against the host loader; `cli augment-preview`."""
import functools
import os

import numpy as np
import pytest
import torch

import aug_cases as AC
import cropcache_cases as CC
from openglottal_amd import augment as A
from openglottal_amd import cli

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def twin(S, case, tile):
    im, mk = AC.tiles(S)
    oi, om = A.augment_host(im, mk, [tile], AC.records(S)[case:case + 1])
    return oi[0], om[0]


def device_tiles(S):
    im, mk = AC.tiles(S)
    return torch.from_numpy(im.copy()).cuda(), torch.from_numpy(mk.copy()).cuda()


def held(aug, dim, dmk, S, cases, idx):
    recs = AC.records(S)[cases]
    oi, om = aug.batch(dim, dmk, idx, recs)
    assert oi.dtype == om.dtype == torch.float32 and tuple(oi.shape) == tuple(om.shape) == (len(idx), 1, S, S) and oi.is_cuda
    oi, om = oi.cpu().numpy(), om.cpu().numpy()
    for k, (c, n) in enumerate(zip(cases, idx)):
        wi, wm = twin(S, int(c), int(n))
        cid = AC.case_list(S)[int(c)][0]
        assert np.array_equal(oi[k].view(np.uint32), wi.view(np.uint32)), (S, cid, n, float(np.abs(oi[k] - wi).max()))
        assert np.array_equal(om[k], wm), (S, cid, n)


@pytest.mark.parametrize("S", AC.SIZES)
def test_device_equals_twin_bit_for_bit(S):
    dim, dmk = device_tiles(S)
    ncases = len(AC.case_list(S))
    aug = A.Augmenter(S)
    for c in range(ncases):                                                   # b = 1
        held(aug, dim, dmk, S, [c], [c % 4])
    for lo in range(0, ncases, 5):                                            # b = 5: every record different, one index repeated
        cases = list(range(lo, min(lo + 5, ncases)))
        held(aug, dim, dmk, S, cases, [3, 0, 2, 1, 0][:len(cases)])
    aug.set_chunk(3)                                                          # b = chunk + 1: two micro-batches
    for lo in range(0, ncases - 3, 4):
        held(aug, dim, dmk, S, list(range(lo, lo + 4)), [1, 1, 3, 0])
    held(aug, dim, dmk, S, list(range(ncases)), [(3 * c + 1) % 4 for c in range(ncases)])     # and the whole list at once
    oi, om = aug.batch(dim, dmk, [2, 0, 2], augment=False)                     # the plain path
    im, mk = AC.tiles(S)
    assert np.array_equal(oi.cpu().numpy()[:, 0], im[[2, 0, 2]].astype(np.float32) / np.float32(255.0))
    assert np.array_equal(om.cpu().numpy()[:, 0], (mk[[2, 0, 2]] > 0).astype(np.float32))
    e, z = aug.batch(dim, dmk, [], [])
    assert tuple(e.shape) == (0, 1, S, S) and tuple(z.shape) == (0, 1, S, S)


def test_an_index_outside_the_tiles_gives_an_all_zero_sample():
    S = 32
    dim, dmk = device_tiles(S)
    aug = A.Augmenter(S)
    for augment in (True, False):
        oi, om = aug.batch(dim, dmk, [-1, 1, 4], [A.record(angle=10)] * 3 if augment else None, augment=augment)
        assert not oi[0].any() and not om[0].any() and not oi[2].any() and not om[2].any() and oi[1].any()


def test_a_samples_tensors_depend_on_seed_epoch_and_sample_only():
    S = 32
    im, mk = AC.tiles(S, 7, 1)
    host = A.CropCacheLoader((im, mk), batch=7, seed=11, decode="host")
    want = {e: host.samples(list(range(7)), e) for e in (0, 1)}
    assert not np.array_equal(want[0][0], want[1][0])
    for chunk in (1, 3, 8):
        for batch in (1, 4):
            dev = A.CropCacheLoader((im, mk), batch=batch, seed=11, decode="device", chunk=chunk)
            for e in (0, 1):
                order, at = dev.order(e), 0
                assert sorted(order) == list(range(7)) and order == host.order(e)
                for oi, om in dev:
                    for k in range(oi.shape[0]):
                        n = order[at]
                        assert np.array_equal(oi[k].cpu().numpy().view(np.uint32), want[e][0][n].view(np.uint32)), (chunk, batch, e, n)
                        assert np.array_equal(om[k].cpu().numpy(), want[e][1][n]), (chunk, batch, e, n)
                        at += 1
                assert at == 7


def test_the_device_loader_equals_the_host_loader(tmp_path):
    S = 32
    im, mk = AC.tiles(S, 12, 2)
    AC.write_cache(str(tmp_path), "train", im, mk)
    for augment in (True, False):
        dev = A.CropCacheLoader(str(tmp_path), "train", batch=5, augment=augment, seed=4, decode="device")
        host = A.CropCacheLoader(str(tmp_path), "train", batch=5, augment=augment, seed=4, decode="host")
        assert np.array_equal(dev.images.cpu().numpy(), im) and np.array_equal(host.masks, mk) and len(dev) == len(host) == 3
        got, want = list(dev), list(host)
        assert [tuple(a.shape) for a, _ in got] == [(5, 1, S, S), (5, 1, S, S), (2, 1, S, S)]
        for (a, b), (c, d) in zip(got, want):
            assert np.array_equal(a.cpu().numpy().view(np.uint32), c.view(np.uint32)) and np.array_equal(b.cpu().numpy(), d)


def test_cli_augment_preview_writes_the_twins_files(tmp_path, capsys):
    S = 32
    im, mk = AC.tiles(S, 5, 3)
    AC.write_cache(str(tmp_path / "cache"), "val", im, mk)
    argv = ["augment-preview", "--cache", str(tmp_path / "cache"), "--split", "val", "--n", "4", "--seed", "9"]
    assert cli.main(argv + ["--out", str(tmp_path / "dev")]) == 0 and "4 augmented pairs" in capsys.readouterr().out
    assert cli.main(argv + ["--out", str(tmp_path / "host"), "--host"]) == 0
    a, b = CC.tree(str(tmp_path / "dev")), CC.tree(str(tmp_path / "host"))
    assert a == b and sorted(a) == sorted(os.path.join(d, f"{k:06d}.png") for d in ("images", "masks") for k in range(4))
    imgs, msks = A.CropCacheLoader(str(tmp_path / "cache"), "val", augment=True, shuffle=False, seed=9, decode="host").samples([0, 1, 2, 3], 0)
    for k in range(4):
        assert np.array_equal(CC.gray_of(str(tmp_path / "dev" / "images" / f"{k:06d}.png")), np.rint(imgs[k, 0] * np.float32(255)).astype(np.uint8))
        assert np.array_equal(CC.gray_of(str(tmp_path / "dev" / "masks" / f"{k:06d}.png")), (msks[k, 0] * 255).astype(np.uint8))
