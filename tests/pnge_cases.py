"""Cases of the PNG encoder tests (tests/test_pnge_*.py, tests/test_gpu_pnge*.py): frames whose RAW streams hold what the segment
coder can get wrong, an independent numpy filter judge, and a walker over a zlib stream that reports every deflate block.

A one-row gray frame built as the running sum of a byte string d (`sub_row`) is filtered with Sub and gives d back, so the raw stream of
such a case is `[1] + d` whatever d holds: runs of exact lengths, Fibonacci literal counts, all 256 literals.  The tests assert that from
the twin's own raw bytes before they rely on it."""
import functools
import heapq
import struct
import zlib

import numpy as np

import png_cases as PC

SEGMENTS = (64, 256, 32768)
RUNS = (1, 2, 3, 4, 258, 259, 260, 261, 262, 517)


def sub_row(d):
    """[1, W, 1] gray whose Sub-filtered row is d"""
    return (np.cumsum(np.asarray(d, np.int64)) % 256).astype(np.uint8).reshape(1, -1, 1)


def smooth(H, W, seed):
    r = np.random.default_rng(seed)
    return ((np.add.outer(np.arange(H) * 3, np.arange(W) * 2) + r.integers(0, 6, (H, W))) % 256).astype(np.uint8)[..., None]


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 1)).astype(np.uint8)


def runs_bytes(lengths, seed=0):
    """zero runs of the given lengths, each behind a byte that is not zero: [7, 0 * L0, 9, 0 * L1, ...]"""
    out = []
    for i, n in enumerate(lengths):
        out += [7 + 2 * (i % 3)] + [0] * n
    return out + [5]


def fibonacci_bytes():
    """28 654 bytes over 20 values, no two neighbours equal.  With the filter-type byte 1 in front of them the counts are the
    Fibonacci numbers 1, 2, 3, 5, ..., 10 946; the end-of-block's 1 completes the sequence, in which every partial sum is below the
    next but one count: each Huffman tree of it is a chain, 20 bits deep"""
    fib = [1, 2]
    while len(fib) < 20:
        fib.append(fib[-1] + fib[-2])
    vals = [0, 1, 255, 2, 254, 3, 253, 4, 252, 5, 251, 6, 250, 7, 249, 8, 248, 9, 247, 10]
    syms = [v for v, n in zip(vals, reversed(fib)) for _ in range(n - (1 if v == 1 else 0))]
    out = [0] * len(syms)
    slots = list(range(0, len(syms), 2)) + list(range(1, len(syms), 2))
    for s, p in zip(syms, slots):
        out[p] = s
    assert all(a != b for a, b in zip(out, out[1:]))
    return out


def all_literals_bytes():
    p = list(np.random.default_rng(11).permutation(256))
    return [int(v) for v in p] + runs_bytes((5, 20, 100, 300, 3000), 1) + [int(v) for v in p[::-1]]


def filters_frame():
    """nine rows of 64: built so that each of the five types wins a row and several rows tie (tests/test_pnge_host.py judges it)"""
    W, r = 64, np.random.default_rng(5)
    x = np.arange(W)
    n1 = r.integers(0, 256, W // 2)
    rows = [x % 2, 100 + 2 * x, 100 + 2 * x + x % 2, np.r_[n1, np.full(W // 2, 40)], np.r_[n1, np.full(W // 2, 90)], 4 * x]
    avg, a = [], 0
    for b in rows[-1]:
        a = (a + int(b)) >> 1
        avg.append(a)
    rows += [np.array(avg), np.zeros(W, int), np.zeros(W, int)]
    return np.stack(rows).astype(np.uint8)[..., None]


def _rgb(g):
    """a C = 3 frame (B G R) from a gray case: three different planes of the same kind"""
    g = g[..., 0]
    return np.ascontiguousarray(np.stack([g, g[::-1, ::-1], np.roll(g, 2, 1)], -1))


def _exact(total, C):
    """(H, W) with H * (1 + W * C) == total, or None"""
    for H in (1, 2, 3, 4, 5, 6, 7, 8):
        if total % H == 0 and (total // H - 1) % C == 0 and total // H - 1 >= C:
            return H, (total // H - 1) // C
    return None


@functools.lru_cache(None)
def gray_cases():
    """[(name, [H,W,1] u8, (S, ...))]"""
    out = [("h1", smooth(1, 37, 1), (64, 32768)), ("w1", smooth(29, 1, 2), (64, 32768)), ("1x1", np.full((1, 1, 1), 200, np.uint8), (64, 32768)),
           ("seam-rows", smooth(5, 40, 3), (64,)),                              # stride 41: rows straddle the seams at 64, 128, 192
           ("zeros-4x50", np.zeros((4, 50, 1), np.uint8), (64, 256)),           # one run across every seam: it must be cut there
           ("zeros-256", np.zeros((256, 256, 1), np.uint8), (32768,)),
           ("runs", sub_row(runs_bytes(RUNS + (32768,))), (64, 256, 32768)),
           ("filters", filters_frame(), (64, 32768)),
           ("noise", noise(64, 70, 4), SEGMENTS),
           ("fibonacci", sub_row(fibonacci_bytes()), (32768,)),
           ("all-literals", sub_row(all_literals_bytes()), (256, 32768)),
           ("two-segments-181x182", smooth(182, 181, 6), (32768,))]          # 182 rows of 1 + 181 bytes: 33 124
    for S in SEGMENTS:
        for total, tag in ((S - 1, "S-1"), (S, "S"), (S + 1, "S+1"), (2 * S, "2S")):
            H, W = _exact(total, 1)
            out.append((f"raw-{tag}-{S}", smooth(H, W, total % 97), (S,)))
    return out


@functools.lru_cache(None)
def synth_frames():
    """(frames, masks): synthetic glottis frames of openglottal_amd.synth at 256 x 256, gray, and their {0,255} ground truth"""
    from openglottal_amd import synth

    return synth.glottis_frames(1, 3, seed=99)


@functools.lru_cache(None)
def crop_tiles():
    """(image tiles, mask tiles) [3,256,256] u8: og_crop_tile_host of the synthetic frames and of their masks, boxes of three aspect
    ratios, so that the tiles carry letterbox padding -- what the crop-training cache holds"""
    import ctypes as C

    from openglottal_amd._lib import check, lib

    fr, gt = synth_frames()
    boxes = ((60, 40, 200, 230), (30, 90, 240, 170), (70, 70, 190, 190))
    out = np.zeros((2, 3, 256, 256), np.uint8)
    for k, src in enumerate((fr, gt)):
        for i, b in enumerate(boxes):
            box = np.array(b, np.int32)
            check(lib().og_crop_tile_host(C.c_void_p(src[i].ctypes.data), 256, 256, 1, C.c_void_p(box.ctypes.data), 256,
                                          C.c_void_p(out[k, i].ctypes.data)), "og_crop_tile_host")
    return out[0], out[1]


@functools.lru_cache(None)
def cases():
    """[(id, frame [H,W,C] u8, S)] at C = 1 and C = 3"""
    out = []
    for name, g, segs in gray_cases():
        for S in segs:
            out.append((f"{name}-c1-s{S}", g, S))
            if not name.startswith("raw-"):
                out.append((f"{name}-c3-s{S}", _rgb(g), S))
    for S in SEGMENTS:
        for total, tag in ((S - 1, "S-1"), (S, "S"), (S + 1, "S+1"), (2 * S, "2S")):
            hw = _exact(total, 3)
            if hw:
                out.append((f"raw-{tag}-{S}-c3-s{S}", _rgb(smooth(hw[0], 3 * hw[1], total % 89))[:, :hw[1]].copy(), S))
    fr = synth_frames()[0]
    for i in range(fr.shape[0]):
        g = np.ascontiguousarray(fr[i].reshape(256, 256, 1))
        out.append((f"synth{i}-c1-s32768", g, 32768))
    out.append(("synth0-c3-s32768", _rgb(np.ascontiguousarray(fr[0].reshape(256, 256, 1))), 32768))
    return out


BY_ID = {}


def by_id(cid):
    if not BY_ID:
        BY_ID.update({c[0]: c for c in cases()})
    return BY_ID[cid]


@functools.lru_cache(None)
def batch(cid):
    """[7,H,W,C]: the case's frame and six variations of it, so that a call at chunk 3 has three micro-batches"""
    f = by_id(cid)[1]
    return np.ascontiguousarray(np.stack([f, f[::-1], f[:, ::-1], f ^ 0x55, np.roll(f, 1, 1), np.zeros_like(f), 255 - f]))


@functools.lru_cache(None)
def host_files(cid):
    """the twin's files of `batch(cid)`: computed once, shared by the GPU tests"""
    from openglottal_amd import png as P

    return tuple(P.encode_host(f, by_id(cid)[2]) for f in batch(cid))


# ── the judges ──────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def unfiltered_rows(frame):
    """[H, rb] u8: the scanlines a PNG of the frame holds (C = 3 frames are B G R, the file R G B)"""
    f = frame[..., ::-1] if frame.shape[2] == 3 else frame
    return np.ascontiguousarray(f).reshape(frame.shape[0], -1)


def filter_costs(frame):
    """[H, 5] int: per row and filter type the sum of |filtered byte as int8|, and [H, 5, rb] the filtered bytes; numpy, independent"""
    rows = unfiltered_rows(frame).astype(np.int64)
    H, rb = rows.shape
    bpp = frame.shape[2]
    up = np.vstack([np.zeros((1, rb), np.int64), rows[:-1]])
    left = np.hstack([np.zeros((H, bpp), np.int64), rows[:, :-bpp]]) if rb > bpp else np.zeros((H, rb), np.int64)
    ul = np.hstack([np.zeros((H, bpp), np.int64), up[:, :-bpp]]) if rb > bpp else np.zeros((H, rb), np.int64)
    p = left + up - ul
    pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    filt = np.stack([rows, rows - left, rows - up, rows - ((left + up) >> 1), rows - paeth], 1) & 255
    cost = np.where(filt < 128, filt, 256 - filt).sum(2)
    return cost, filt.astype(np.uint8)


def raw_reference(frame):
    """the raw stream by the rule of the header, from numpy alone"""
    cost, filt = filter_costs(frame)
    best = cost.argmin(1)                                                  # (argmin takes the first of equals: ties to the lower type)
    return b"".join(bytes([int(t)]) + filt[r, t].tobytes() for r, t in enumerate(best))


def run_lengths(b):
    a = np.frombuffer(bytes(b), np.uint8)
    edges = np.flatnonzero(np.r_[True, a[1:] != a[:-1], True])
    return np.diff(edges), a[edges[:-1]]


def idat(png):
    cs = PC.chunks_of(png)
    assert [t for t, _ in cs][0] == b"IHDR" and cs[-1][0] == b"IEND"
    assert png[:8] == PC.SIG and all(zlib.crc32(t + d) == struct.unpack(">I", png[o:o + 4])[0] for (t, d), o in zip(cs, _crc_offsets(png)))
    return b"".join(d for t, d in cs if t == b"IDAT")


def _crc_offsets(png):
    at, out = 8, []
    while at + 12 <= len(png):
        n, = struct.unpack_from(">I", png, at)
        out.append(at + 8 + n)
        at += 12 + n
    return out


class _Reader:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def bits(self, k):
        v = 0
        for i in range(k):
            v |= ((self.d[self.pos >> 3] >> (self.pos & 7)) & 1) << i
            self.pos += 1
        return v

    def sym(self, table):
        code, n = 0, 0
        while True:
            code = (code << 1) | self.bits(1)
            n += 1
            if (n, code) in table:
                return table[(n, code)]
            assert n < 16, "bits that are no code"


def _table(lens):
    return {(l, c): s for s, (c, l) in PC.canon(list(lens)).items()}


def blocks(z):
    """every deflate block of a zlib stream: dict(type, final, start (bit), end (bit), n (bytes it produces), lit_lens, dist_lens,
    tokens [(length or 0, literal)]) -- a plain inflate of RFC 1951 for stored and dynamic blocks, for the tests to look inside"""
    r, out = _Reader(z[2:]), []
    while True:
        b = {"start": r.pos, "final": r.bits(1), "type": r.bits(2), "n": 0, "tokens": []}
        if b["type"] == 0:
            r.pos = (r.pos + 7) & ~7
            n, nn = r.bits(16), r.bits(16)
            assert n ^ nn == 0xFFFF
            b["n"], b["data"] = n, bytes(r.d[r.pos >> 3:(r.pos >> 3) + n])
            r.pos += 8 * n
        else:
            assert b["type"] == 2, "only stored and dynamic blocks are written"
            hlit, hdist, hclen = r.bits(5) + 257, r.bits(5) + 1, r.bits(4) + 4
            cl = [0] * 19
            for i in range(hclen):
                cl[PC.CL_ORDER[i]] = r.bits(3)
            b["cl_lens"], t, lens = cl, _table(cl), []
            while len(lens) < hlit + hdist:
                s = r.sym(t)
                if s < 16:
                    lens.append(s)
                elif s == 16:
                    lens += [lens[-1]] * (3 + r.bits(2))
                else:
                    lens += [0] * (3 + r.bits(3) if s == 17 else 11 + r.bits(7))
            assert len(lens) == hlit + hdist, "a repeat past the end"
            b["lit_lens"], b["dist_lens"] = lens[:hlit], lens[hlit:]
            lt, dt = _table(b["lit_lens"]), _table(b["dist_lens"])
            while True:
                s = r.sym(lt)
                if s == 256:
                    break
                if s < 256:
                    b["tokens"].append((0, s))
                    b["n"] += 1
                else:
                    length = PC.LBASE[s - 257] + r.bits(PC.LEXT[s - 257])
                    assert r.sym(dt) == 0
                    b["tokens"].append((length, None))
                    b["n"] += length
        b["end"] = r.pos
        out.append(b)
        if b["final"]:
            return out


def kraft(lens):
    return sum(2.0 ** -l for l in lens if l)


def huffman_depth(freq):
    """the depth of an unlimited Huffman code"""
    heap = [(f, i, 0) for i, f in enumerate(freq) if f]
    heapq.heapify(heap)
    tick = len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tick, max(a[2], b[2]) + 1))
        tick += 1
    return heap[0][2]


def corpus_blob():
    """the case list for tools/pnge_host_check.cpp: u32 count, then per case u32 H, W, C, S and the frame's bytes"""
    cs = cases()
    return struct.pack("<I", len(cs)) + b"".join(struct.pack("<IIII", *f.shape, S) + f.tobytes() for _, f, S in cs)
