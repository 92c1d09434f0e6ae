"""Inputs of the JPEG decoder's tests (helper module, like tests/mjpeg_cases.py): Pillow-encoded files of seeded noise in every accepted
form, and the hostile corpus -- truncations, single-byte substitutions and damaged restart markers of two small 4:2:0 files -- that
tests/test_mjpd_host.py holds the twin to, tools/mjpd_host_fuzz.cpp runs under sanitizers, and tests/test_gpu_mjpd.py takes its
status cases from.  Everything is cached: a file is encoded once per process."""
import functools
import io

import numpy as np
from PIL import Image

from openglottal_amd import mjpeg as MJ

FORMS = {"gray": None, "444": 0, "422": 1, "420": 2}          # Pillow's `subsampling`
SAMPLING = {"gray": 0, "444": 1, "422": 2, "420": 3}          # the header's `sampling`
LISTED = set(range(1, 6))                                      # statuses a damaged scan may end with


@functools.lru_cache(maxsize=None)
def noise(H, W, seed=0):
    a = np.random.default_rng([H, W, seed]).integers(0, 256, (H, W, 3), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def pillow_jpeg(H, W, form, quality=75, restart=0, optimize=False, seed=0):
    """Seeded noise (smooth images never reach the long codes) as a baseline JPEG file; `restart`: MCUs per restart interval."""
    im = Image.fromarray(noise(H, W, seed))
    kw = {"quality": quality, "optimize": optimize}
    if form == "gray":
        im = im.convert("L")
    else:
        kw["subsampling"] = FORMS[form]
    if restart:
        kw["restart_marker_blocks"] = restart
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def pillow_bgr(jpeg):
    return MJ.decode_jpeg_bgr(jpeg)


@functools.lru_cache(maxsize=None)
def twin(jpeg):
    """`(frame or None, status)` of the host twin, computed once per file."""
    f, st = MJ.decode_host(jpeg, statuses=True)
    if f is not None:
        f.setflags(write=False)
    return f, st


def scan_span(jpeg):
    i = MJ.parse(jpeg)
    return i["scan_offset"], i["scan_offset"] + i["scan_length"]


def strip_dht(jpeg):
    """The file without its DHT segments."""
    out, at = bytearray(jpeg[:2]), 2
    while jpeg[at + 1] != 0xDA:
        n = 2 + ((jpeg[at + 2] << 8) | jpeg[at + 3])
        if jpeg[at + 1] != 0xC4:
            out += jpeg[at:at + n]
        at += n
    return bytes(out + jpeg[at:])


def rst_positions(jpeg):
    lo, hi = scan_span(jpeg)
    return [i for i in range(lo, hi - 1) if jpeg[i] == 0xFF and 0xD0 <= jpeg[i + 1] <= 0xD7]


@functools.lru_cache(maxsize=None)
def bases():
    """The two files of the hostile corpus: 17x9 4:2:0 with Ri = 1, and without DRI."""
    return pillow_jpeg(17, 9, "420", 75, 1), pillow_jpeg(17, 9, "420", 75, 0)


@functools.lru_cache(maxsize=None)
def hostile():
    """`[(label, bytes)]`: every truncation, 500 seeded substitutions in the scan, and a removed, a doubled and a renumbered RSTm."""
    out = []
    for name, j in zip(("ri1", "nodri"), bases()):
        out += [(f"{name}-cut{n}", j[:n]) for n in range(len(j))]
        lo, hi = scan_span(j)
        rng = np.random.default_rng(len(j))
        for k in range(500):
            b = bytearray(j)
            at = int(rng.integers(lo, hi))
            b[at] = int(rng.integers(0, 256))
            out.append((f"{name}-sub{k}@{at}", bytes(b)))
    j = bases()[0]
    r = rst_positions(j)
    assert len(r) == 1                                          # two MCUs, Ri = 1: one RST0
    out.append(("ri1-rst-removed", j[:r[0]] + j[r[0] + 2:]))
    out.append(("ri1-rst-doubled", j[:r[0]] + j[r[0]:r[0] + 2] + j[r[0]:]))
    out.append(("ri1-rst-renumbered", j[:r[0] + 1] + b"\xd3" + j[r[0] + 2:]))
    return out


@functools.lru_cache(maxsize=None)
def status_cases():
    """From the corpus, for the GPU's status batch: a file truncated mid-scan (status 1), one with an invalid code (2), one whose
    RSTm is missing (5); all of the Ri = 1 base, so one call holds them next to the intact file."""
    corpus = dict(hostile())
    j = bases()[0]
    lo, hi = scan_span(j)
    cut = corpus[f"ri1-cut{(rst_positions(j)[0] + 2 + hi) // 2}"]          # inside the last interval: the RSTm count still holds
    assert twin(cut)[1] == 1
    invalid = next(b for label, b in hostile() if label.startswith("ri1-sub") and twin(b)[1] == 2)
    missing = corpus["ri1-rst-removed"]
    assert twin(missing)[1] == 5
    return j, cut, invalid, missing
