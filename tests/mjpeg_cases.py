"""Shared cases and independent models for include/openglottal_hip_mjpeg.h (helper module, like tests/overlay_cases.py).

* ``decode_scan``: a pure-Python baseline JPEG reader -- marker walk, DQT / SOF0 / DHT / DRI / SOS parse, Huffman decode to zigzag
  coefficients.  It shares no code with the library and ASSERTS what a lenient decoder forgives: every restart interval ends in at
  most 7 one-bits of padding, RSTm follows in order, EOI comes directly after the last interval, and a 0xFF inside the scan is
  followed only by 0x00 or the expected marker.
* ``model_quotients``: float64 -- the JFIF matrix, the exact DCT, the division by q, unrounded.
* ``CASES``: the seeded matrix, parametrised by Ri = og_mjpeg_limit(1), and ``host_files``: the host twin's files, computed once.
  ``test_mjpeg_host.py::test_the_matrix_fires`` asserts that the matrix really contains a stuffed 0xFF, a ZRL, an AC amplitude of
  category 10, a DC difference of category 11 and a file of odd length.
"""
import collections
import functools
import io
import struct

import numpy as np

from openglottal_amd import mjpeg as MJ

Case = collections.namedtuple("Case", "id frames quality")


def zigzag():
    """natural index of zigzag position k, walked along the anti-diagonals"""
    order = []
    for s in range(15):
        rng = range(max(0, s - 7), min(7, s) + 1)
        for y in (rng if s % 2 else reversed(rng)):
            order.append(y * 8 + (s - y))
    return order


ZZ = zigzag()


# ── the reader ────────────────────────────────────────────────────────────────────────────────────────────────────────
def parse(jpeg: bytes):
    """Headers of a baseline file: dict with H, W, comps [(id, sampling, tq)], q {id: [64] natural}, dht [(class, id, bits, vals)],
    ri, sos [(id, td, ta)], and ``scan``: the offset of the entropy-coded data."""
    assert jpeg[:2] == b"\xff\xd8", "no SOI"
    at, out = 2, {"q": {}, "dht": [], "ri": 0, "segments": []}
    while True:
        assert jpeg[at] == 0xFF, f"no marker at byte {at}"
        m = jpeg[at + 1]
        n = (jpeg[at + 2] << 8) | jpeg[at + 3]
        body = jpeg[at + 4:at + 2 + n]
        out["segments"].append((m, bytes(jpeg[at:at + 2 + n])))
        if m == 0xDB:
            p = 0
            while p < len(body):
                assert body[p] >> 4 == 0, "16-bit quantisation table in a baseline file"
                tab = [0] * 64
                for k in range(64):
                    tab[ZZ[k]] = body[p + 1 + k]
                out["q"][body[p] & 15] = tab
                p += 65
        elif m == 0xC0:
            assert body[0] == 8
            out["H"], out["W"] = (body[1] << 8) | body[2], (body[3] << 8) | body[4]
            out["comps"] = [(body[6 + 3 * i], body[7 + 3 * i], body[8 + 3 * i]) for i in range(body[5])]
        elif m == 0xC4:
            p = 0
            while p < len(body):
                bits = list(body[p + 1:p + 17])
                vals = list(body[p + 17:p + 17 + sum(bits)])
                out["dht"].append((body[p] >> 4, body[p] & 15, bits, vals))
                p += 17 + sum(bits)
        elif m == 0xDD:
            out["ri"] = (body[0] << 8) | body[1]
        elif m == 0xDA:
            out["sos"] = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(body[0])]
            assert tuple(body[1 + 2 * body[0]:]) == (0, 63, 0), "not a sequential baseline scan"
            out["scan"] = at + 2 + n
            return out
        else:
            assert 0xE0 <= m <= 0xEF or m == 0xFE, f"unexpected marker {m:#x}"
        at += 2 + n


def _codes(bits, vals):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


def decode_scan(jpeg: bytes):
    """``(header dict, coefficients int [M,3,64] zigzag, stats)``.  stats: Counter with 'stuffed', 'zrl', 'eob', ('ac', category),
    ('dc', category), 'intervals'."""
    h = parse(jpeg)
    assert [c[1] for c in h["comps"]] == [0x11] * 3 and len(h["sos"]) == 3, "not 4:4:4 with three components"
    H, W, ri = h["H"], h["W"], h["ri"]
    M = ((H + 7) // 8) * ((W + 7) // 8)
    assert ri > 0
    n_int = (M + ri - 1) // ri
    # split the scan into intervals on its markers
    at, intervals, cur, stats = h["scan"], [], bytearray(), collections.Counter()
    while True:
        b = jpeg[at]
        if b != 0xFF:
            cur.append(b)
            at += 1
            continue
        nxt = jpeg[at + 1]
        if nxt == 0:
            cur.append(0xFF)
            stats["stuffed"] += 1
            at += 2
            continue
        intervals.append(bytes(cur))
        cur = bytearray()
        if len(intervals) == n_int:
            assert nxt == 0xD9, f"interval {n_int - 1} is followed by {nxt:#x}, not EOI"
            assert at + 2 == len(jpeg), "bytes after EOI"
            break
        assert nxt == 0xD0 + ((len(intervals) - 1) & 7), f"interval {len(intervals) - 1} is followed by {nxt:#x}"
        at += 2
    stats["intervals"] = n_int
    dc = {i: _codes(b, v) for c, i, b, v in h["dht"] if c == 0}
    ac = {i: _codes(b, v) for c, i, b, v in h["dht"] if c == 1}
    sel = {cid: (td, ta) for cid, td, ta in h["sos"]}
    coefs = np.zeros((M, 3, 64), np.int64)
    for k, data in enumerate(intervals):
        nbits = len(data) * 8
        bit = np.unpackbits(np.frombuffer(data, np.uint8)).tolist()
        pos = 0

        def take(n):
            nonlocal pos
            assert pos + n <= nbits, f"interval {k} ends inside a code"
            v = 0
            for b in bit[pos:pos + n]:
                v = (v << 1) | b
            pos += n
            return v

        def symbol(table):
            code = 0
            for length in range(1, 17):
                code = (code << 1) | take(1)
                if (length, code) in table:
                    return table[(length, code)]
            raise AssertionError(f"interval {k}: no Huffman code matches at bit {pos}")

        def extend(v, n):
            return v if n == 0 or v >> (n - 1) else v - (1 << n) + 1

        pred = [0, 0, 0]
        for m in range(k * ri, min((k + 1) * ri, M)):
            for c, (cid, _, _) in enumerate(h["comps"]):
                td, ta = sel[cid]
                cat = symbol(dc[td])
                assert cat <= 11
                stats[("dc", cat)] += 1
                pred[c] += extend(take(cat), cat)
                coefs[m, c, 0] = pred[c]
                i = 1
                while i < 64:
                    s = symbol(ac[ta])
                    run, cat = s >> 4, s & 15
                    if cat == 0:
                        if run == 15:
                            stats["zrl"] += 1
                            i += 16
                            assert i < 64, "ZRL runs past the block"
                            continue
                        assert run == 0, "EOBn in a baseline scan"
                        stats["eob"] += 1
                        break
                    assert cat <= 10
                    i += run
                    assert i < 64, "run past the block"
                    stats[("ac", cat)] += 1
                    coefs[m, c, i] = extend(take(cat), cat)
                    i += 1
        left = nbits - pos
        assert left < 8 and take(left) == (1 << left) - 1, f"interval {k}: {left} bits of padding, not all ones"
    return h, coefs, stats


# ── the float64 model ─────────────────────────────────────────────────────────────────────────────────────────────────
JFIF = np.array([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]])     # rows Y Cb Cr on R G B
DCT = np.array([[(np.sqrt(0.5) if u == 0 else 1.0) / 2 * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])


def model_coefficients(frame) -> np.ndarray:
    """float64 [M,3,64] zigzag: the exact DCT of the exact JFIF components (level shifted), unquantised"""
    f = np.asarray(frame, np.float64)
    H, W = f.shape[:2]
    f = np.pad(f, ((0, -H % 8), (0, -W % 8), (0, 0)), mode="edge")
    ycc = f[..., ::-1] @ JFIF.T
    ycc[..., 0] -= 128.0
    my, mx = f.shape[0] // 8, f.shape[1] // 8
    blocks = ycc.reshape(my, 8, mx, 8, 3).transpose(0, 2, 4, 1, 3).reshape(my * mx, 3, 8, 8)
    c = DCT @ blocks @ DCT.T
    return c.reshape(my * mx, 3, 64)[..., ZZ]


def model_quotients(frame, qlum, qchroma) -> np.ndarray:
    q = np.stack([np.asarray(qlum, np.float64)[ZZ], np.asarray(qchroma, np.float64)[ZZ], np.asarray(qchroma, np.float64)[ZZ]])
    return model_coefficients(frame) / q[None]


def error_bound() -> float:
    """E of the header's ERROR BOUND paragraph, from the widths stated there: 4 fraction bits in the samples, 16-bit colour constants,
    14-bit DCT constants, 6 fraction bits after pass 1, 4 after pass 2.  In coefficient units."""
    fixed = np.array([[19595, 38470, 7471], [-11059, -21709, 32768], [32768, -27439, -5329]], np.float64)
    e_s = 1 / 32 + 255 * np.abs(fixed / 65536 - JFIF).sum(1).max()
    A = np.abs(DCT).sum(1).max()
    pass1 = (8 * 0.5 * 2048 / 2 ** 12 + 0.5) / 64
    pass2 = 8 * 0.5 * (np.abs(DCT).sum(1).max() * 128 * 64 + 2.5) / 2 ** 20
    return A * A * e_s + A * pass1 + pass2 + 1 / 32


# ── the case matrix ───────────────────────────────────────────────────────────────────────────────────────────────────
def _ramp(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(40 + xx * 150 // max(W - 1, 1)), (30 + yy * 200 // max(H - 1, 1)), (20 + (xx + yy) * 100 // max(H + W - 2, 1))], -1).astype(np.uint8)


def _noise(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def _columns(H, W):
    """sign(cos((2x+1) 4 pi / 16)) at the u8 extremes along x: the largest AC coefficient there is"""
    row = np.where(np.cos((2 * (np.arange(W) % 8) + 1) * 4 * np.pi / 16) > 0, 255, 0).astype(np.uint8)
    return np.broadcast_to(row[None, :, None], (H, W, 3)).copy()


def _steps(H, W):
    """8x8 blocks alternately black and white: DC differences of +-2040 at quality 100"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.broadcast_to(((((yy // 8) + (xx // 8)) % 2) * 255).astype(np.uint8)[..., None], (H, W, 3)).copy()


def _high(H, W):
    """the (7,7) basis function alone: 62 zeros in front of one coefficient, so three ZRL"""
    c = np.cos((2 * (np.arange(8)) + 1) * 7 * np.pi / 16)
    yy, xx = np.mgrid[0:H, 0:W]
    v = np.clip(np.rint(128 + 120 * c[yy % 8] * c[xx % 8]), 0, 255).astype(np.uint8)
    return np.broadcast_to(v[..., None], (H, W, 3)).copy()


def _overlay_like(H, W):
    """a frame as k_overlay leaves it: gray, a one-pixel green outline, a one-pixel yellow rectangle (BGR)"""
    f = np.full((H, W, 3), 0, np.uint8)
    f[...] = (96 + (np.arange(W) * 64 // max(W, 1)))[None, :, None]
    y0, y1, x0, x1 = H // 4, max(H // 4, 3 * H // 4 - 1), W // 4, max(W // 4, 3 * W // 4 - 1)
    f[y0, x0:x1 + 1] = f[y1, x0:x1 + 1] = (0, 220, 255)
    f[y0:y1 + 1, x0] = f[y0:y1 + 1, x1] = (0, 220, 255)
    yy, xx = np.mgrid[0:H, 0:W]
    r2 = (yy - H / 2) ** 2 + (xx - W / 2) ** 2
    rad = min(H, W) / 5
    ring = (r2 <= rad ** 2) & (r2 > max(rad - 1.2, 0) ** 2)
    f[ring] = (0, 255, 0)
    fill = r2 <= max(rad - 1.2, 0) ** 2
    f[fill, 1] = np.minimum(255, f[fill, 1].astype(int) + 102).astype(np.uint8)
    return f


def build_cases():
    ri = MJ.limit(1)
    one = lambda f: f[None]
    cases = []
    add = lambda cid, frames, q: cases.append(Case(cid, np.ascontiguousarray(frames), q))
    # shapes: H, W
    shapes = {"1x1": (1, 1), "8x8": (8, 8), "13x21": (13, 21), "ri": (8, 8 * ri), "ri+1": (8, 8 * ri + 8), "ragged": (40, 8 * ri // 2 - 3),
              "wrap": (80, 8 * ri - 8), "wide": (16, 720)}
    assert ((40 + 7) // 8) * ((8 * ri // 2 - 3 + 7) // 8) % ri != 0 and 10 * (ri - 1) > 8 * ri      # ragged; more than 8 intervals
    for name, (H, W) in shapes.items():
        add(f"{name}-zero", one(np.zeros((H, W, 3), np.uint8)), 75)
        add(f"{name}-255", one(np.full((H, W, 3), 255, np.uint8)), 75)
        add(f"{name}-ramp", one(_ramp(H, W)), 75)
        add(f"{name}-noise-q100", one(_noise(H, W, H * 31 + W)), 100)
        add(f"{name}-columns-q100", one(_columns(H, W)), 100)
        add(f"{name}-rows-q100", one(_columns(W, H).transpose(1, 0, 2)), 100)
        add(f"{name}-overlay", one(_overlay_like(H, W)), 75)
    add("13x21-steps-q100", one(_steps(13, 21)), 100)
    add("wrap-steps-q100", one(_steps(80, 8 * ri - 8)), 100)
    add("ragged-high", one(_high(40, 8 * ri // 2 - 3)), 75)
    add("ragged-noise-q1", one(_noise(40, 8 * ri // 2 - 3, 5)), 1)
    add("ragged-noise-q50", one(_noise(40, 8 * ri // 2 - 3, 6)), 50)
    add("256-ramp", one(_ramp(256, 256)), 75)
    add("256-overlay-q90", one(_overlay_like(256, 256)), 90)
    add("256-noise-q100", one(_noise(256, 256, 9)), 100)
    H, W = 40, 56
    add("batch7", np.stack([np.zeros((H, W, 3), np.uint8), _noise(H, W, 1), _ramp(H, W), _overlay_like(H, W), _steps(H, W), _high(H, W),
                            np.full((H, W, 3), 255, np.uint8)]), 75)
    return cases


CASES = build_cases()
IDS = [c.id for c in CASES]
BY_ID = {c.id: c for c in CASES}


@functools.lru_cache(maxsize=None)
def host_files(cid: str):
    """the host twin's file of every frame of a case: computed once per process, never changed"""
    c = BY_ID[cid]
    return tuple(MJ.encode_host(f, c.quality) for f in c.frames)


@functools.lru_cache(maxsize=None)
def decoded(cid: str):
    return tuple(decode_scan(j) for j in host_files(cid))


def pillow_decode(jpeg: bytes) -> np.ndarray:
    """BGR u8, with LOAD_TRUNCATED_IMAGES off: a short or damaged scan is an error"""
    from PIL import Image, ImageFile

    assert ImageFile.LOAD_TRUNCATED_IMAGES is False
    im = Image.open(io.BytesIO(jpeg))
    im.load()
    assert im.mode == "RGB"
    return np.asarray(im)[..., ::-1]


def pillow_encode(frame, qlum, qchroma) -> bytes:
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(np.asarray(frame)[..., ::-1])).save(b, "JPEG", qtables=[list(map(int, qlum)), list(map(int, qchroma))],
                                                                         subsampling=0)
    return b.getvalue()


def psnr(a, b) -> float:
    mse = ((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2).mean()
    return float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


def riff_walk(data, lo, hi, depth=0):
    """[(fourcc or list type, payload offset, size, children or None)]: every chunk must end inside its parent, on an even offset"""
    out, at = [], lo
    while at < hi:
        assert at % 2 == 0 and at + 8 <= hi, (at, hi)
        cc, n = struct.unpack_from("<4sI", data, at)
        assert at + 8 + n <= hi, (cc, at, n, hi)
        if cc in (b"RIFF", b"LIST"):
            out.append((data[at + 8:at + 12], at + 8, n, riff_walk(data, at + 12, at + 8 + n, depth + 1)))
        else:
            out.append((cc, at + 8, n, None))
        at += 8 + n + (n & 1)
    assert at == hi, (at, hi)                                             # a parent's size includes its children's pad bytes
    return out
