"""The crop trainer's data path on the device (include_enc/openglottal_hip_aug.h): what `CroppedGlottisDataset` /
`GTCroppedGlottisDataset.__getitem__` + `_tensor_and_augment` (`scripts/train_unet_crop.py:167-214`, `:303-349`; the same chain in
`openglottal/data.py:284-329`) do per sample on a `DataLoader` worker.  The cache's tiles stay resident as two ``[N,S,S]`` u8 tensors;
one call turns a list of sample indices into the augmented f32 ``[b,1,S,S]`` image and mask batch that ``model(imgs)`` consumes.

``draw`` consumes a ``random.Random`` in exactly the reference's order and returns the sample's record (``PARAMS``, the 64 bytes of
``og_aug_params``): only numbers the host drew or computed.  ``Augmenter`` wraps one ``og_aug`` handle; ``augment_host`` is its twin,
bit for bit.  ``CropCacheLoader`` stands in for the trainer's two ``DataLoader``s: a sample's record and noise key depend only on
(seed, epoch, sample number), so its tensors do not depend on the batch size, the chunk or its place in the epoch.
The noise has the distribution of ``torch.randn_like``, not its numbers; parity with torchvision itself is unpinned (the header)."""
from __future__ import annotations

import ctypes as C
import json
import math
import os
import random

import numpy as np

from . import png as P
from ._lib import OpenGlottalHipError, check, lib, ptr

PARAMS = np.dtype([("flips", "<u4"), ("cos_t", "<f4"), ("sin_t", "<f4"), ("new_size", "<i4"), ("noise_sigma", "<f4"), ("ks", "<i4"),
                   ("noise_key", "<u8"), ("k1", "<f4", (5,)), ("brightness", "<f4"), ("contrast", "<f4"), ("reserved", "<u4")])
assert PARAMS.itemsize == 64
STAGES = {"flip": 1, "rotate": 2, "rescale": 3, "noise": 4, "blur": 5, "brightness": 6, "contrast": 7}
_M64 = (1 << 64) - 1


def limit(which: int) -> int:
    return int(lib().og_aug_limit(which))


def blur_kernel(ks: int, sigma: float) -> np.ndarray:
    """torchvision's `_get_gaussian_kernel1d` in f32: exp(-0.5 (x / sigma)^2) over linspace(-(ks-1)/2, (ks-1)/2, ks), over its sum."""
    half = (int(ks) - 1) * 0.5
    x = np.linspace(-half, half, int(ks), dtype=np.float32)
    pdf = np.exp(np.float32(-0.5) * np.square(x / np.float32(sigma)), dtype=np.float32)
    return (pdf / pdf.sum(dtype=np.float32)).astype(np.float32)


def draw_values(rng: random.Random, S: int) -> dict:
    """The reference's draws, in its order (`train_unet_crop.py:171-203`): what was drawn, ``None`` for a stage left out."""
    v = {"hflip": rng.random() > 0.5, "vflip": rng.random() > 0.5, "angle": rng.uniform(-30, 30)}
    v["new_size"] = int(int(S) * rng.uniform(0.85, 1.15)) if rng.random() > 0.5 else None
    v["noise_sigma"] = rng.uniform(0.01, 0.05) if rng.random() > 0.5 else None
    if rng.random() > 0.5:
        v["ks"] = rng.choice([3, 5])
        v["blur_sigma"] = rng.uniform(0.5, 1.5)
    else:
        v["ks"] = v["blur_sigma"] = None
    v["brightness"] = rng.uniform(0.7, 1.3) if rng.random() > 0.5 else None
    v["contrast"] = rng.uniform(0.7, 1.3) if rng.random() > 0.5 else None
    return v


def record(hflip=False, vflip=False, angle=0.0, new_size=None, noise_sigma=None, ks=None, blur_sigma=None, brightness=None, contrast=None,
           noise_key=0):
    """One ``PARAMS`` record from drawn values; ``None`` (or 0) leaves a stage off."""
    r = np.zeros(1, PARAMS)[0]
    r["flips"] = (1 if hflip else 0) | (2 if vflip else 0)
    t = math.radians(float(angle))
    r["cos_t"], r["sin_t"] = math.cos(t), math.sin(t)
    r["new_size"] = int(new_size or 0)
    r["noise_sigma"] = float(noise_sigma or 0.0)
    if ks:
        r["ks"] = int(ks)
        r["k1"][:int(ks)] = blur_kernel(ks, blur_sigma)
    r["brightness"] = float(brightness or 0.0)
    r["contrast"] = float(contrast or 0.0)
    r["noise_key"] = int(noise_key) & _M64
    return r


def draw(rng: random.Random, S: int, noise_key: int = 0):
    """Consumes ``rng`` exactly as one `_tensor_and_augment` call does and returns the sample's record."""
    return record(noise_key=noise_key, **draw_values(rng, S))


def records(recs) -> np.ndarray:
    """A list of records (or an array of them) as one contiguous ``PARAMS`` array."""
    if isinstance(recs, np.ndarray) and recs.dtype == PARAMS:
        return np.ascontiguousarray(recs).reshape(-1)
    return np.array(list(recs), dtype=PARAMS).reshape(-1)


def _mix(x: int) -> int:
    x &= _M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sample_key(seed: int, epoch: int, sample: int, salt: int = 0) -> int:
    """64 bits that depend on (seed, epoch, sample, salt) only."""
    k = _mix(int(seed) + 0x9E3779B97F4A7C15)
    k = _mix(k ^ (int(epoch) + 1) * 0xD1B54A32D192ED03)
    k = _mix(k ^ (int(sample) + 1) * 0x8CB92BA72F3D8DD7)
    return _mix(k ^ (int(salt) * 0x9E3779B97F4A7C15))


def sample_record(seed: int, epoch: int, sample: int, S: int):
    """The record of one sample of one epoch: ``draw`` on a generator seeded by ``sample_key``, the noise key another such key."""
    return draw(random.Random(sample_key(seed, epoch, sample, 1)), S, noise_key=sample_key(seed, epoch, sample, 2))


def noise_host(key: int, n: int) -> np.ndarray:
    out = np.empty(int(n), np.float32)
    check(lib().og_aug_noise_host(C.c_uint64(int(key) & _M64), int(n), ptr(out)), "og_aug_noise_host")
    return out


def stage_host(stage, img: np.ndarray, msk, rec):
    """One stage (a name of ``STAGES`` or 1..7) of the twin: ``img`` f32 ``[S,S]``, ``msk`` u8 ``[S,S]`` of 0/1 or None ->
    ``(img, msk)``."""
    a = np.ascontiguousarray(img, np.float32)
    m = None if msk is None else np.ascontiguousarray(msk, np.uint8)
    S = a.shape[0]
    if a.shape != (S, S) or (m is not None and m.shape != (S, S)):
        raise OpenGlottalHipError(f"the planes must be square and alike, not {a.shape}")
    r = records([rec])
    out = np.empty_like(a)
    om = None if m is None else np.empty_like(m)
    check(lib().og_aug_stage_host(int(STAGES.get(stage, stage)), ptr(a), ptr(m), S, ptr(r), ptr(out), ptr(om)), "og_aug_stage_host")
    return out, om


def _tiles(a, what: str) -> np.ndarray:
    a = np.ascontiguousarray(a, np.uint8)
    if a.ndim != 3 or a.shape[1] != a.shape[2]:
        raise OpenGlottalHipError(f"{what} must be [N,S,S] u8, not {a.shape}")
    return a


def augment_host(images, masks, idx, recs=None, augment: bool = True):
    """The twin composition on numpy arrays: ``images``, ``masks`` ``[N,S,S]`` u8 -> ``(imgs, msks)`` f32 ``[b,1,S,S]``."""
    im, mk = _tiles(images, "images"), _tiles(masks, "masks")
    if im.shape != mk.shape:
        raise OpenGlottalHipError(f"images are {im.shape}, masks {mk.shape}")
    idx = [int(i) for i in idx]
    r = records(recs) if augment else None
    if augment and len(r) != len(idx):
        raise OpenGlottalHipError(f"{len(idx)} indices but {len(r)} records")
    S = im.shape[1]
    oi, om = np.empty((len(idx), 1, S, S), np.float32), np.empty((len(idx), 1, S, S), np.float32)
    for k, n in enumerate(idx):
        if not 0 <= n < im.shape[0]:
            raise OpenGlottalHipError(f"index {n} outside the {im.shape[0]} tiles")
        check(lib().og_aug_apply_host(ptr(im[n]), ptr(mk[n]), S, ptr(r[k:k + 1]) if augment else None, 1 if augment else 0, ptr(oi[k]), ptr(om[k])),
              "og_aug_apply_host")
    return oi, om


class Augmenter:
    """One ``og_aug`` handle: resident u8 tiles and sample indices in, augmented f32 batches out, all on the device."""

    def __init__(self, crop_size: int = 256, chunk: int = 128):
        self.crop_size = int(crop_size)
        self._h = lib().og_aug_create()
        if not self._h:
            raise OpenGlottalHipError("og_aug_create failed")
        self.set_chunk(chunk)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                lib().og_aug_destroy(h)
            except Exception:
                pass

    def set_chunk(self, chunk: int) -> None:
        check(lib().og_aug_set_chunk(self._h, int(chunk)), "og_aug_set_chunk")
        self.chunk = int(chunk)

    def sync(self) -> None:
        check(lib().og_aug_sync(self._h), "og_aug_sync")

    def batch(self, images_dev, masks_dev, idx, recs=None, augment: bool = True):
        """``images_dev``, ``masks_dev``: ``[N,S,S]`` u8 CUDA tensors; ``idx``: the samples (a list, an array or an int32 CUDA tensor),
        repeats allowed; ``recs``: their records.  Returns two float32 CUDA tensors ``[b,1,S,S]``.  Waited for."""
        import torch

        N, S = int(images_dev.shape[0]), self.crop_size
        if tuple(images_dev.shape) != (N, S, S) or tuple(masks_dev.shape) != (N, S, S):
            raise OpenGlottalHipError(f"tiles must be [N,{S},{S}], not {tuple(images_dev.shape)} and {tuple(masks_dev.shape)}")
        if not torch.is_tensor(idx):
            idx = torch.as_tensor(np.asarray(idx, np.int32).reshape(-1), device=images_dev.device)
        idx = idx.to(torch.int32).contiguous()
        b = int(idx.numel())
        r = records(recs) if augment else None
        if augment and len(r) != b:
            raise OpenGlottalHipError(f"{b} indices but {len(r)} records")
        imgs = torch.empty((b, 1, S, S), dtype=torch.float32, device=images_dev.device)
        msks = torch.empty((b, 1, S, S), dtype=torch.float32, device=images_dev.device)
        torch.cuda.synchronize()   # (the handle runs on a stream of its own)
        check(lib().og_aug_batch_u8_dev(self._h, ptr(images_dev), ptr(masks_dev), N, S, ptr(idx), ptr(r) if augment else None, b,
                                        1 if augment else 0, ptr(imgs), ptr(msks)), "og_aug_batch_u8_dev")
        self.sync()
        return imgs, msks

    def plan(self, b: int, augment: bool = True):
        return plan(b, self.crop_size, self.chunk, augment)


def plan(b: int, S: int, chunk: int = 128, augment: bool = True):
    """Dry run of ``Augmenter.batch``: ``(records, workspace_bytes)``; a record is a dict of the plan line's fields."""
    out = C.create_string_buffer(1 << 20)
    ws = C.c_longlong()
    n = lib().og_aug_plan(int(b), int(S), int(chunk), 1 if augment else 0, out, len(out), C.byref(ws))
    if n < 0:
        check(n, "og_aug_plan")
    names = ("kernel", "gx", "gy", "gz", "block", "lds", "workspace", "counters", "writes")
    recs = [{k: (v if k in ("kernel", "writes") else int(v)) for k, v in zip(names, line.split("|"))} for line in out.value.decode().splitlines()]
    assert len(recs) == n
    return recs, ws.value


def _read_cache(cache_dir, split: str, device: bool):
    base = os.path.join(os.fspath(cache_dir), split)
    try:
        with open(os.path.join(base, "meta.json")) as fh:
            meta = json.loads(fh.read())
        n, S = int(meta["n"]), int(meta["crop_size"])
    except (OSError, ValueError, KeyError, TypeError) as e:
        raise OpenGlottalHipError(f"{base} holds no usable meta.json: {e}") from e
    planes = []
    for sub in ("images", "masks"):
        d = os.path.join(base, sub)
        names = sorted(f for f in os.listdir(d) if f.endswith(".png")) if os.path.isdir(d) else []
        if names != [f"{k:06d}.png" for k in range(n)]:
            raise OpenGlottalHipError(f"meta.json states n = {n}, but {d} holds {len(names)} .png files (or other names than %06d.png)")
        files = [P._read(os.path.join(d, f)) for f in names]
        for k, f in enumerate(files):
            info = P.parse(f)
            if info["status"] or (info["H"], info["W"]) != (S, S):
                raise OpenGlottalHipError(f"meta.json states crop_size = {S}, but {sub}/{names[k]} is {info['H']} x {info['W']}"
                                          + (f" ({info.get('why', '')})" if info["status"] else ""))
        if device:
            planes.append(P.PngDecoder().decode_resident(files, 1).reshape(n, S, S))
        else:
            planes.append(np.stack([P.decode_host(f, 1)[..., 0] for f in files]))
    return planes[0], planes[1]


class CropCacheLoader:
    """The trainer's loader over one split of a crop cache (``cropcache.build``), or over in-memory ``(images, masks)`` ``[N,S,S]`` u8
    arrays (the full-frame trainer's case).  Iterating it runs one epoch and yields ``(imgs, msks)`` ``[b,1,S,S]`` float32: CUDA
    tensors with ``decode="device"``, numpy arrays from the host twin with ``decode="host"`` -- the same bits.  ``epoch`` counts the
    iterations begun; ``set_epoch`` sets it."""

    def __init__(self, cache_dir, split: str = "train", batch: int = 16, augment: bool = True, shuffle: bool = True, seed: int = 0,
                 decode: str = "device", chunk: int = 128):
        if decode not in ("device", "host"):
            raise OpenGlottalHipError("decode must be 'device' or 'host'")
        if int(batch) < 1:
            raise OpenGlottalHipError("batch must be positive")
        self.device = decode == "device"
        if isinstance(cache_dir, (tuple, list)):
            images, masks = cache_dir
            if self.device:
                import torch

                images, masks = ((a if torch.is_tensor(a) else torch.from_numpy(np.array(a, dtype=np.uint8))).to("cuda").contiguous()
                                 for a in (images, masks))
            else:
                images, masks = _tiles(images, "images"), _tiles(masks, "masks")
        else:
            images, masks = _read_cache(cache_dir, split, self.device)
        if images.ndim != 3 or images.shape[1] != images.shape[2] or tuple(images.shape) != tuple(masks.shape):
            raise OpenGlottalHipError(f"tiles must be two [N,S,S] u8 arrays, not {tuple(images.shape)} and {tuple(masks.shape)}")
        self.images, self.masks = images, masks
        self.n, self.crop_size = int(images.shape[0]), int(images.shape[1])
        self.batch, self.augment, self.shuffle, self.seed, self.epoch = int(batch), bool(augment), bool(shuffle), int(seed), 0
        self.augmenter = Augmenter(self.crop_size, chunk) if self.device else None

    def __len__(self) -> int:
        return -(-self.n // self.batch)

    def set_epoch(self, epoch: int) -> None:
        self.epoch = int(epoch)

    def order(self, epoch: int) -> list:
        """The samples of an epoch in the order they are yielded."""
        order = list(range(self.n))
        if self.shuffle:
            random.Random(sample_key(self.seed, epoch, -1, 3)).shuffle(order)
        return order

    def samples(self, idx, epoch: int):
        """The batch of the given samples as they come out in ``epoch``."""
        recs = records([sample_record(self.seed, epoch, n, self.crop_size) for n in idx]) if self.augment else None
        if self.device:
            return self.augmenter.batch(self.images, self.masks, idx, recs, self.augment)
        return augment_host(self.images, self.masks, idx, recs, self.augment)

    def __iter__(self):
        epoch, self.epoch = self.epoch, self.epoch + 1
        order = self.order(epoch)
        for at in range(0, self.n, self.batch):
            yield self.samples(order[at:at + self.batch], epoch)


def preview(cache_dir, split: str, n: int, seed: int, out_dir, host: bool = False) -> int:
    """`cli augment-preview`: the first ``n`` samples of epoch 0, augmented, as ``out_dir/images|masks/%06d.png``: images
    ``round(I * 255)``, masks ``M * 255``, coded by ``PngEncoder`` (``host``: by the twins)."""
    loader = CropCacheLoader(cache_dir, split, batch=max(int(n), 1), augment=True, shuffle=False, seed=seed, decode="host" if host else "device")
    k = min(int(n), loader.n)
    imgs, msks = loader.samples(list(range(k)), 0)
    if host:
        tiles = [np.rint(imgs[:, 0] * np.float32(255.0)).astype(np.uint8), (msks[:, 0] * 255).astype(np.uint8)]
        files = [[P.encode_host(t) for t in plane] for plane in tiles]
    else:
        import torch

        tiles = [torch.round(imgs[:, 0] * 255.0).to(torch.uint8).contiguous(), (msks[:, 0] * 255).to(torch.uint8).contiguous()]
        enc = P.PngEncoder()
        files = [enc.files_resident(t, k, loader.crop_size, loader.crop_size, 1) if k else [] for t in tiles]
    for sub, fs in zip(("images", "masks"), files):
        os.makedirs(os.path.join(out_dir, sub), exist_ok=True)
        for i, data in enumerate(fs):
            with open(os.path.join(out_dir, sub, f"{i:06d}.png"), "wb") as fh:
                fh.write(data)
    return k
