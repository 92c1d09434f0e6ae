"""Tiles, the case list and the torch oracles of the augmentation tests (tests/test_aug_host.py, tests/test_gpu_aug.py,
tests/test_gpu_aug_extents.py, tools/aug_cases_corpus.py).  The oracles are the torch functionals the rule of
include_enc/openglottal_hip_aug.h reduces to, composed as torchvision composes them (restated here: torchvision is not installed)."""
import functools
import math

import numpy as np

SIZES = (32, 37, 64)
NOISE_KEY = 0x5EED0A06                                                        # chosen once, on the CPU


@functools.lru_cache(maxsize=None)
def tiles(S, N=4, seed=0):
    """(images, masks) [N,S,S] u8: a smooth pattern with noise, borders that are not zero; elliptic labels of 1 or 255, one empty."""
    r = np.random.default_rng(100 * S + seed)
    yy, xx = np.mgrid[0:S, 0:S]
    imgs, msks = [], []
    for n in range(N):
        img = 120 + 60 * np.sin(xx / 4.0 + n) + 40 * np.cos(yy / 3.0 - n) + r.normal(0, 12, (S, S))
        imgs.append(np.clip(img, 0, 255).astype(np.uint8))
        m = np.zeros((S, S), np.uint8)
        if n != 2:
            m[((yy - S / 2 - n) / (S / 5.0)) ** 2 + ((xx - S / 2 + 2 * n) / (S / 3.0)) ** 2 <= 1.0] = 255 if n % 2 else 1
            m[0, :3] = m[-1, -2:] = 255                                       # label pixels on the first and the last row
        msks.append(m)
    imgs[-1][0, :] = 255                                                      # a bright first row and last column: what a neighbour tile
    imgs[-1][:, -1] = 255                                                     # or the slack would have to look like to be noticed
    a, b = np.stack(imgs), np.stack(msks)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def angles(S):
    """0, +-30, 17.3 and 90 degrees.  sin 30 = 1/2 exactly, and at an odd S the centred coordinates are integers: the column X = 0 then
    lies on ties of the mask's rounding, 2.6 % of the pixels at S = 37, more than the 1 % a case may leave out -- 29.5 stands in there."""
    a = 29.5 if S % 2 else 30
    return (0, a, -a, 17.3, 90)


def case_list(S):
    """[(id, keyword arguments of augment.record)]: one stage at a time at the values of the issue, every stage off, all of them on."""
    out = [(f"angle{a}", {"angle": a}) for a in angles(S)]
    out += [(f"flip{int(h)}{int(v)}", {"hflip": h, "vflip": v}) for h in (False, True) for v in (False, True)]
    out += [(f"size{n}", {"new_size": n}) for n in (int(0.85 * S), S - 1, S, S + 1, int(1.15 * S))]
    out += [(f"blur{k}-{s}", {"ks": k, "blur_sigma": s}) for k in (3, 5) for s in (0.5, 1.5)]
    out += [(f"bright{f}", {"brightness": f}) for f in (0.7, 1.3)] + [(f"contrast{f}", {"contrast": f}) for f in (0.7, 1.3)]
    out += [("noise", {"noise_sigma": 0.03, "noise_key": NOISE_KEY}), ("off", {})]
    out += [("all", {"hflip": True, "vflip": True, "angle": angles(S)[2], "new_size": int(1.15 * S), "noise_sigma": 0.05, "noise_key": NOISE_KEY + 1,
                     "ks": 5, "blur_sigma": 1.1, "brightness": 1.3, "contrast": 0.7}),
            ("all-small", {"hflip": True, "angle": angles(S)[1], "new_size": int(0.85 * S), "noise_sigma": 0.01, "noise_key": NOISE_KEY + 2, "ks": 3,
                           "blur_sigma": 0.7, "brightness": 0.7, "contrast": 1.3})]
    return out


def records(S):
    from openglottal_amd import augment as A

    return A.records([A.record(**kw) for _, kw in case_list(S)])


# ── the oracles ─────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def rotate_grid(S, angle, dtype):
    """torchvision's `_gen_affine_grid` for `rotate(img, angle)` of an S x S image: theta = [[cos, -sin, 0], [sin, cos, 0]] of
    radians(angle) (the inverse matrix of `_get_inverse_affine_matrix(center 0, -angle)`)."""
    import torch

    t = math.radians(angle)
    theta = torch.tensor([[math.cos(t), -math.sin(t), 0.0], [math.sin(t), math.cos(t), 0.0]], dtype=dtype)[None]
    base = torch.empty(1, S, S, 3, dtype=dtype)
    line = torch.linspace(-S * 0.5 + 0.5, S * 0.5 + 0.5 - 1, steps=S, dtype=dtype)
    base[..., 0].copy_(line)
    base[..., 1].copy_(line.unsqueeze(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * S, 0.5 * S], dtype=dtype)
    return base.view(1, S * S, 3).bmm(rescaled).view(1, S, S, 2)


def torch_rotate(plane, angle, mode):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(plane, np.float32))
    grid = rotate_grid(t.shape[-1], angle, torch.float32)
    return torch.nn.functional.grid_sample(t[None, None], grid, mode=mode, padding_mode="zeros", align_corners=False)[0, 0].numpy()


def source_coordinates(S, angle):
    """(sx, sy) in f64: the source index of every output pixel."""
    t = math.radians(angle)
    i, j = np.mgrid[0:S, 0:S].astype(np.float64)
    X, Y = j + 0.5 - S / 2, i + 0.5 - S / 2
    return math.cos(t) * X - math.sin(t) * Y + (S - 1) / 2, math.sin(t) * X + math.cos(t) * Y + (S - 1) / 2


def fit(t, S):
    """The reference's crop or pad of a resized plane back to S x S."""
    import torch

    n = t.shape[-1]
    if n > S:
        off = (n - S) // 2
        return t[..., off:off + S, off:off + S]
    pad = S - n
    pl, pr = pad // 2, pad - pad // 2
    return torch.nn.functional.pad(t, [pl, pr, pl, pr])


def torch_rescale(plane, new_size, mode):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(plane, np.float32))[None, None]
    kw = {"mode": "bilinear", "align_corners": False, "antialias": True} if mode == "bilinear" else {"mode": "nearest"}
    return fit(torch.nn.functional.interpolate(t, size=(new_size, new_size), **kw), plane.shape[-1])[0, 0].numpy()


def torch_blur(plane, k1):
    """torchvision's gaussian_blur: reflect padding, conv2d with mm(k1[:, None], k1[None, :])."""
    import torch

    k = torch.from_numpy(np.ascontiguousarray(k1, np.float32))
    r = k.numel() // 2
    t = torch.nn.functional.pad(torch.from_numpy(np.ascontiguousarray(plane, np.float32))[None, None], [r, r, r, r], mode="reflect")
    return torch.nn.functional.conv2d(t, torch.mm(k[:, None], k[None, :])[None, None])[0, 0].numpy()


def write_cache(directory, split, images, masks, crop_size=None, n=None):
    """A crop cache as `cropcache.build` lays it out, from given tiles: <split>/images|masks/%06d.png (the encoder's twin) and meta.json."""
    import json
    import os

    from openglottal_amd import png as P

    for sub, planes in (("images", images), ("masks", masks)):
        os.makedirs(os.path.join(directory, split, sub), exist_ok=True)
        for k, t in enumerate(planes):
            with open(os.path.join(directory, split, sub, f"{k:06d}.png"), "wb") as fh:
                fh.write(P.encode_host(t))
    meta = {"n": len(images) if n is None else n, "crop_size": int(images.shape[1]) if crop_size is None else crop_size, "label_suffix": "",
            "source_hash": "0" * 16, "roi_mode": "gt"}
    with open(os.path.join(directory, split, "meta.json"), "w") as fh:
        fh.write(json.dumps(meta, indent=2))
    return meta


def corpus():
    """[(S, record, image [S,S] u8, mask [S,S] u8)]: the case list at every size, case k on tile k mod N"""
    out = []
    for S in SIZES:
        im, mk = tiles(S)
        for k, rec in enumerate(records(S)):
            out.append((S, rec, im[k % im.shape[0]], mk[k % im.shape[0]]))
    return out


def corpus_blob():
    """The input of tools/aug_host_check.cpp: u32 count, then per case u32 S, the 64 bytes of the record, S * S image bytes, S * S mask
    bytes (little endian)."""
    cs = corpus()
    parts = [np.uint32(len(cs)).tobytes()]
    for S, rec, im, mk in cs:
        parts += [np.uint32(S).tobytes(), rec.tobytes(), im.tobytes(), mk.tobytes()]
    return b"".join(parts)
