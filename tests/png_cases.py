"""Cases of the PNG decoder tests (tests/test_png_*.py, tests/test_gpu_png*.py): a token-level deflate WRITER (stored, fixed and
dynamic blocks from explicit literal / (length, distance) tokens and explicit code lengths), a PNG assembler (filter type per row,
IDAT split at any byte, CRCs from zlib.crc32), an independent numpy decoder over zlib.decompress, the valid set and the hostile corpus.
Every stream meant to be valid is checked with zlib.decompress where it is made, every stream meant to be invalid must make zlib raise.
The ring files (ring_files, deep_errors) put matches, stored blocks and errors on the seams of the decoder's 32 KiB window; lz_expand,
match_facts, token_spans and writers give the plain meaning of their tokens, from which tests/test_png_host.py asserts each seam."""
import functools
import heapq
import io
import struct
import zlib

import numpy as np
from PIL import Image

LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
DEXT = [0, 0, 0, 0] + [d // 2 - 1 for d in range(4, 30)]
DBASE = [1, 2, 3, 4] + [1 + ((2 + (d & 1)) << (d // 2 - 1)) for d in range(4, 30)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
SAMPLES = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
FORMS = [(0, 1), (0, 2), (0, 4), (0, 8), (3, 1), (3, 2), (3, 4), (3, 8), (2, 8), (4, 8), (6, 8)]


# ── bits and codes ──────────────────────────────────────────────────────────────────────────────────────────────────────────────────
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, k):
        """k bits of v, least significant first (every field of a deflate stream that is no Huffman code)"""
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, l):
        """a Huffman code, most significant bit first"""
        for i in range(l - 1, -1, -1):
            self.put((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bitpos(self):
        return 8 * len(self.out) + self.n

    def bytes(self):
        self.align()
        return bytes(self.out)


def canon(lens):
    """{symbol: (code, length)} of RFC 1951 3.2.2; nothing is checked, so over-subscribed and incomplete sets can be written"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def huffman_lengths(freq, maxlen=15):
    """code lengths of a complete code over the symbols with freq > 0 (at least two symbols get a code)"""
    used = [s for s, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(used) == 1:
        used.append(0 if used[0] else 1)
    heap = [(freq[s] or 1, i, [s]) for i, s in enumerate(used)]
    heapq.heapify(heap)
    tick = len(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    assert max(lens) <= maxlen, "flatten the frequencies"
    return lens


def len_sym(length):
    return max(s for s in range(29) if LBASE[s] <= length) if length < 258 else 28


def dist_sym(dist):
    return max(d for d in range(30) if DBASE[d] <= dist)


def token_syms(tokens):
    """(litlen symbols, distance symbols) the tokens use"""
    ls, ds = [256], []
    for t in tokens:
        if isinstance(t, int):
            ls.append(t)
        elif t[0] == "L":
            ls.append(t[1])
        elif t[0] == "D":
            ls.append(257 + len_sym(t[1]))
            ds.append(t[2])
        else:
            ls.append(257 + len_sym(t[0]))
            ds.append(dist_sym(t[1]))
    return ls, ds


def put_tokens(w, tokens, lit, dist, eob=True):
    """tokens: a literal (int), (length, distance), ("L", litlen symbol) without extra bits, ("D", length, distance symbol) without
    the distance's extra bits"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*lit[t])
        elif t[0] == "L":
            w.code(*lit[t[1]])
        else:
            length = t[1] if t[0] == "D" else t[0]
            s = len_sym(length)
            w.code(*lit[257 + s])
            w.put(length - LBASE[s], LEXT[s])
            if t[0] == "D":
                w.code(*dist[t[2]])
            else:
                d = dist_sym(t[1])
                w.code(*dist[d])
                w.put(t[1] - DBASE[d], DEXT[d])
    if eob:
        w.code(*lit[256])


def stored(w, data, final=False, nlen=None):
    w.put(1 if final else 0, 1)
    w.put(0, 2)
    w.align()
    w.put(len(data), 16)
    w.put((~len(data) & 0xFFFF) if nlen is None else nlen, 16)
    w.out += bytes(data)


def fixed(w, tokens, final=False, eob=True):
    w.put(1 if final else 0, 1)
    w.put(1, 2)
    put_tokens(w, tokens, canon(FIXED_LIT), canon(FIXED_DIST), eob)


def dynamic(w, tokens, final=False, lit_lens=None, dist_lens=None, cl_lens=None, cl_seq=None, repeats=True, eob=True, hlit=None, hdist=None):
    """lit_lens / dist_lens: explicit code lengths (lists; trailing zeros are cut to HLIT >= 257, HDIST >= 1), else a Huffman code of
    the tokens' symbols.  cl_seq: the explicit (symbol, extra value) list of the code-length sequence, else its run-length coding
    (repeats) or one symbol per length.  cl_lens: explicit lengths of the code-length code."""
    ls, ds = token_syms(tokens)
    if lit_lens is None:
        f = [0] * 286
        for s in ls:
            f[s] += 1
        lit_lens = huffman_lengths(f)
    if dist_lens is None:
        f = [0] * 30
        for s in ds:
            f[s] += 1
        dist_lens = [0] if not ds else ([1 if s == ds[0] else 0 for s in range(30)] if len(set(ds)) == 1 else huffman_lengths(f))
    lit_lens, dist_lens = list(lit_lens), list(dist_lens)
    while len(lit_lens) > 257 and lit_lens[-1] == 0:
        lit_lens.pop()
    while len(dist_lens) > 1 and dist_lens[-1] == 0:
        dist_lens.pop()
    lit_lens += [0] * (257 - len(lit_lens))
    nl, nd = (len(lit_lens) if hlit is None else hlit), (len(dist_lens) if hdist is None else hdist)
    seq = lit_lens + dist_lens
    if cl_seq is None:
        cl_seq, i = [], 0
        while i < len(seq):
            v, run = seq[i], 1
            while i + run < len(seq) and seq[i + run] == v:
                run += 1
            if repeats and v == 0 and run >= 3:
                k = min(run, 138)
                cl_seq.append((17, k - 3) if k <= 10 else (18, k - 11))
            elif repeats and run >= 4:
                k = min(run - 1, 6)
                cl_seq += [(v, 0), (16, k - 3)]
                k += 1
            else:
                k = 1
                cl_seq.append((v, 0))
            i += k
    if cl_lens is None:
        f = [0] * 19
        for s, _ in cl_seq:
            f[s] += 1
        cl_lens = huffman_lengths(f, 7)
    hclen = max(4, max((i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]), default=4))
    w.put(1 if final else 0, 1)
    w.put(2, 2)
    w.put(nl - 257, 5)
    w.put(nd - 1, 5)
    w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_lens[CL_ORDER[i]], 3)
    cl = canon(cl_lens)
    for s, extra in cl_seq:
        w.code(*cl[s])
        if s >= 16:
            w.put(extra, {16: 2, 17: 3, 18: 7}[s])
    put_tokens(w, tokens, canon(lit_lens), canon(dist_lens), eob)


def zwrap(deflate, raw=None, header=b"\x78\x9c", adler=None):
    a = zlib.adler32(raw) if adler is None else adler
    return header + bytes(deflate) + struct.pack(">I", a & 0xFFFFFFFF)


def zstream(build, raw, **kw):
    """a zlib stream from `build(w)` that must inflate to raw"""
    w = Bits()
    build(w)
    z = zwrap(w.bytes(), raw, **kw)
    assert zlib.decompress(z) == bytes(raw)
    return z


def zbad(build, raw=b"", **kw):
    """a zlib stream that zlib must refuse"""
    w = Bits()
    build(w)
    z = zwrap(w.bytes(), raw, **kw)
    try:
        zlib.decompress(z)
    except zlib.error:
        return z
    raise AssertionError("zlib accepts a stream meant to be invalid")


# ── the PNG assembler ───────────────────────────────────────────────────────────────────────────────────────────────────────────────
def chunk(t, d):
    return struct.pack(">I", len(d)) + t + d + struct.pack(">I", zlib.crc32(t + d))


SIG = b"\x89PNG\r\n\x1a\n"


def row_bytes(W, ctype, depth):
    return (W * SAMPLES[ctype] * depth + 7) // 8


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def filter_rows(rows, filters, bpp):
    """unfiltered scanlines -> the raw bytes of the zlib stream, filter type filters[r] for row r"""
    out, prev = bytearray(), bytes(len(rows[0]))
    for row, ft in zip(rows, filters):
        out.append(ft)
        for x, v in enumerate(row):
            a = row[x - bpp] if x >= bpp else 0
            b, c = prev[x], (prev[x - bpp] if x >= bpp else 0)
            out.append((v - (0, a, b, (a + b) >> 1, paeth(a, b, c))[ft]) & 255)
        prev = row
    return bytes(out)


def assemble(H, W, ctype, depth, z, plte=None, cuts=None, idat=None, extra=(), after=(), interlace=0, ihdr=None, end=True):
    """z: the zlib stream; cuts: byte positions where IDAT is split; idat: a fixed payload size instead (0: an empty chunk between
    every two 1-byte chunks); extra: chunks before IDAT, after: chunks after it"""
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, ctype, 0, 0, interlace) if ihdr is None else ihdr)
    for c in extra:
        out += c
    if plte is not None:
        out += chunk(b"PLTE", plte)
    if idat is not None:
        parts = [z[i:i + max(idat, 1)] for i in range(0, len(z), max(idat, 1))]
        if idat == 0:
            parts = [p for q in parts for p in (q, b"")]
    else:
        edges = [0] + sorted(cuts or []) + [len(z)]
        parts = [z[a:b] for a, b in zip(edges, edges[1:])]
    for p in parts:
        out += chunk(b"IDAT", p)
    for c in after:
        out += c
    return out + (chunk(b"IEND", b"") if end else b"")


def rng_rows(H, W, ctype, depth, seed=0, smooth=False):
    """H scanlines of random (or slowly varying) samples"""
    r = np.random.default_rng(seed)
    rb = row_bytes(W, ctype, depth)
    if smooth:
        a = (np.add.outer(np.arange(H) * 3, np.arange(rb) * 2) + r.integers(0, 4, (H, rb))) & 255
    else:
        a = r.integers(0, 256, (H, rb))
    return [bytes(x) for x in a.astype(np.uint8)]


def palette(n, seed=0):
    return bytes(np.random.default_rng(100 + seed).integers(0, 256, 3 * n).astype(np.uint8))


def simple(H, W, ctype, depth, filters=None, seed=0, level=6, plte=None, **kw):
    """a file of random rows through zlib.compress"""
    rows = rng_rows(H, W, ctype, depth, seed, kw.pop("smooth", False))
    bpp = max(1, SAMPLES[ctype] * depth // 8)
    raw = filter_rows(rows, filters if filters is not None else [(r + seed) % 5 for r in range(H)], bpp)
    if ctype == 3 and plte is None:
        plte = palette(1 << depth if depth < 8 else 200, seed)
    return assemble(H, W, ctype, depth, zlib.compress(raw, level), plte, **kw)


def pillow_png(H, W, ctype, depth, level, seed=0):
    """a Pillow-written file of the form (gray at depth 2 and 4, which Pillow does not write: the assembler's, zlib at `level`)"""
    r = np.random.default_rng(seed)
    b = io.BytesIO()
    if ctype == 0:
        if depth == 8:
            im = Image.fromarray((np.add.outer(np.arange(H), np.arange(W)) * 5 + r.integers(0, 3, (H, W))).astype(np.uint8), "L")
            im.save(b, "PNG", compress_level=level)
        elif depth == 1:
            Image.fromarray(r.integers(0, 2, (H, W)).astype(bool)).save(b, "PNG", compress_level=level)
        else:                                                     # (Pillow writes no gray file at depth 2 or 4: assembled here, zlib at that level)
            return simple(H, W, 0, depth, None, seed, level)
    elif ctype == 3:
        im = Image.fromarray(r.integers(0, 1 << depth, (H, W)).astype(np.uint8), "P")
        im.putpalette(palette(1 << depth, seed))
        im.save(b, "PNG", compress_level=level, bits=depth)
    else:
        mode = {2: "RGB", 4: "LA", 6: "RGBA"}[ctype]
        a = (np.add.outer(np.arange(H) * 2, np.arange(W) * 3)[..., None] + r.integers(0, 5, (H, W, SAMPLES[ctype]))).astype(np.uint8)
        Image.fromarray(a, mode).save(b, "PNG", compress_level=level)
    return b.getvalue()


# ── the independent decoder: zlib.decompress, a numpy unfilter, an expansion ────────────────────────────────────────────────────────────
def chunks_of(png):
    at, out = 8, []
    while at + 12 <= len(png):
        n, = struct.unpack_from(">I", png, at)
        out.append((png[at + 4:at + 8], png[at + 8:at + 8 + n]))
        at += 12 + n
    return out


def reference(png, C=3):
    """[H,W,C] u8 of a valid file: zlib.decompress of the joined IDAT payloads, unfiltered and expanded here"""
    cs = chunks_of(png)
    W, H, depth, ctype = struct.unpack(">IIBB", cs[0][1][:10])
    plte = next((d for t, d in cs if t == b"PLTE"), b"")
    raw = np.frombuffer(zlib.decompress(b"".join(d for t, d in cs if t == b"IDAT")), np.uint8)
    ns = SAMPLES[ctype]
    rb, bpp = row_bytes(W, ctype, depth), max(1, ns * depth // 8)
    raw = raw[:H * (1 + rb)].reshape(H, 1 + rb)
    rows = np.zeros((H + 1, rb + bpp), np.int32)                 # a zero row above and bpp zero bytes to the left
    for r in range(H):
        ft, line, up = int(raw[r, 0]), raw[r, 1:].astype(np.int32), rows[r]
        cur = rows[r + 1]
        if ft == 0:
            cur[bpp:] = line
        elif ft == 2:
            cur[bpp:] = (line + up[bpp:]) & 255
        else:
            for x in range(rb):
                a, b, c = int(cur[x]), int(up[x + bpp]), int(up[x])
                pred = a if ft == 1 else (a + b) // 2 if ft == 3 else paeth(a, b, c)
                cur[x + bpp] = (int(line[x]) + pred) & 255
    data = rows[1:, bpp:].astype(np.uint8)
    if depth < 8:
        bits = np.unpackbits(data, axis=1)[:, :W * depth].reshape(H, W, depth)
        s = (bits * (1 << np.arange(depth - 1, -1, -1))).sum(-1)
    else:
        s = data.reshape(H, W, ns)
    if ctype == 0:
        rgb = np.repeat((s.reshape(H, W, 1) * (255 // ((1 << depth) - 1))).astype(np.uint8), 3, 2)
    elif ctype == 3:
        table = np.zeros((256, 3), np.uint8)
        table[:len(plte) // 3] = np.frombuffer(plte, np.uint8).reshape(-1, 3)
        rgb = table[s.reshape(H, W)]
    elif ctype == 4:
        rgb = np.repeat(s[..., :1], 3, 2)
    else:
        rgb = s[..., :3]
    bgr = np.ascontiguousarray(rgb[..., ::-1]).astype(np.uint8)
    if C == 3:
        return bgr
    if ctype in (0, 4):
        return bgr[..., :1].copy()
    b, g, r = (bgr[..., i].astype(np.int32) for i in range(3))
    return ((b * 3735 + g * 19235 + r * 9798 + (1 << 14)) >> 15).astype(np.uint8)[..., None]


def pillow(png, gray=False):
    """Pillow's pixels: convert("RGB") reversed to B G R, or convert("L") as [H,W,1]"""
    im = Image.open(io.BytesIO(png))
    im.load()
    return np.asarray(im.convert("L"))[..., None].copy() if gray else np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1])


def is_gray(png):
    return png[25] in (0, 4)


# ── the valid set ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def gray_file(H, W, build, raw, **kw):
    """an 8-bit gray file whose zlib stream comes from the token writer; raw: H * (1 + W) bytes with valid filter types"""
    assert len(raw) == H * (1 + W) and all(raw[r * (1 + W)] <= 4 for r in range(H))
    return assemble(H, W, 0, 8, zstream(build, raw), **kw)


def far_match_file():
    """182 x 183 gray: 32 768 literals, one match of 258 bytes at distance 32 768, literals to the end"""
    H, W = 182, 183
    n = H * (W + 1)
    raw = bytearray(np.random.default_rng(7).integers(0, 256, n).astype(np.uint8))
    for r in range(H):
        raw[r * (W + 1)] = r % 5
    raw[168] = raw[32936]                                        # the match copies byte 168 onto row 179's filter type
    raw[32768:32768 + 258] = raw[0:258]
    toks = list(raw[:32768]) + [(258, 32768)] + list(raw[32768 + 258:])
    return gray_file(H, W, lambda w: fixed(w, toks, True), bytes(raw))


# ── the ring files: matches and stored blocks on the seams of k_png_inflate's 32 KiB window ────────────────────────────────────────────
WINDOW = 32768


def lz_expand(tokens):
    """the plain LZ77 meaning of a token list, byte by byte and with no ring: a literal (int), a stored run ("S", bytes), a match
    (length, distance)"""
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif t[0] == "S":
            out += t[1]
        else:
            for _ in range(t[0]):
                out.append(out[len(out) - t[1]])
    return bytes(out)


def token_spans(tokens):
    """[(pos, length)] of every token"""
    pos, out = 0, []
    for t in tokens:
        n = 1 if isinstance(t, int) else len(t[1]) if t[0] == "S" else t[0]
        out.append((pos, n))
        pos += n
    return out


def match_facts(tokens):
    """[(pos, len, dist)] of every match"""
    return [(p, t[0], t[1]) for t, (p, _) in zip(tokens, token_spans(tokens)) if not isinstance(t, int) and t[0] != "S"]


def writers(tokens):
    """the index of the token that wrote each output byte"""
    return np.concatenate([np.full(n, i, np.int64) for i, (_, n) in enumerate(token_spans(tokens))])


def ring_ft(r):
    return (0, 2, 0, 2, 1, 0, 2, 3, 0, 2, 4)[r % 11]                  # (mostly the two types the numpy unfilter does a row at a time)


def ring_fill(shape, H, W, seed, force=None):
    """shape: blocks ("stored", n) | ("fixed", items) | ("dynamic", items), items ("lit", n) | (length, distance) -> the same blocks with
    bytes in them and the H * (1 + W) raw bytes they mean.  Every byte is seeded random except the row starts (ring_ft) and the bytes
    a match copies onto a row start, which take that row's filter type; force {pos: value} sets the origin of a byte after that."""
    stride, N = 1 + W, H * (1 + W)
    origin, pos = np.arange(N), 0
    for b in shape:
        for it in ([("lit", b[1])] if b[0] == "stored" else b[1]):
            if it[0] == "lit":
                pos += it[1]
            else:
                for _ in range(it[0]):
                    origin[pos] = origin[pos - it[1]]
                    pos += 1
    assert pos == N, (pos, N)
    base = np.random.default_rng(seed).integers(0, 256, N).astype(np.uint8)
    for r in range(H):
        base[origin[r * stride]] = ring_ft(r)
    for p, v in (force or {}).items():
        base[origin[p]] = v
    raw = base[origin].tobytes()
    blocks, pos = [], 0
    for b in shape:
        if b[0] == "stored":
            blocks.append(("stored", raw[pos:pos + b[1]]))
            pos += b[1]
            continue
        toks = []
        for it in b[1]:
            if it[0] == "lit":
                toks += list(raw[pos:pos + it[1]])
                pos += it[1]
            else:
                toks.append(it)
                pos += it[0]
        blocks.append((b[0], toks))
    assert lz_expand(block_tokens(blocks)) == raw
    return blocks, raw


def block_tokens(blocks):
    return [t for b in blocks for t in ([("S", b[1])] if b[0] == "stored" else b[1])]


def write_blocks(w, blocks, final=True, kw=None, marks=None):
    """the blocks in order, the last one final; kw {block index: arguments of `dynamic`}; marks, a list, receives per block
    (bit position of its header, byte position of a stored block's data or None)"""
    for i, b in enumerate(blocks):
        last, at = final and i == len(blocks) - 1, w.bitpos()
        if b[0] == "stored":
            stored(w, b[1], last)
        elif b[0] == "fixed":
            fixed(w, b[1], last)
        else:
            dynamic(w, b[1], last, **(kw or {}).get(i, {}))
        if marks is not None:
            marks.append((at, len(w.out) - len(b[1]) if b[0] == "stored" else None))


def token_bitpos(blocks, bi, ti):
    """the bit of the deflate data at which token ti of the fixed block bi starts"""
    w = Bits()
    write_blocks(w, blocks[:bi], final=False)
    fixed(w, blocks[bi][1][:ti], False, eob=False)
    return w.bitpos()


class Ring:
    def __init__(self, name, H, W, blocks, raw):
        self.name, self.H, self.W, self.blocks, self.raw, self.marks = name, H, W, blocks, raw, []
        self.tokens = block_tokens(blocks)
        self.file = gray_file(H, W, lambda w: write_blocks(w, blocks, marks=self.marks), raw)
        self.z = stream_of(self.file)

    def block_pos(self, bi):
        return sum(n for _, n in token_spans(block_tokens(self.blocks[:bi])))


R4_GAPS = (1, 63, 64, 65, 100, 257)
R5_DISTS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 257)


def _pad(shape, N):
    used = sum(b[1] if b[0] == "stored" else sum(it[1] if it[0] == "lit" else it[0] for it in b[1]) for b in shape)
    return shape + [("stored", N - used)]


@functools.lru_cache(None)
def ring_files():
    """{name: Ring}: 8-bit gray files from the token writer, bulk in stored blocks, each holding the seams its name states
    (tests/test_png_host.py asserts from the tokens that it does)"""
    lit, out = (lambda n: ("lit", n)), {}

    def add(name, H, W, shape, seed):
        out[name] = Ring(name, H, W, *ring_fill(_pad(shape, H * (1 + W)) if shape[-1][0] != "dynamic" else shape, H, W, seed))

    # R1: a match out of a stored block in the first window; a stored block across the wrap point and a match out of both its sides
    add("ring-stored-match", 172, 199, [("stored", 600), ("fixed", [(258, 300), lit(10)]), ("stored", 31000), ("stored", 2000),
                                        ("fixed", [(258, 1200), lit(6)])], 31)
    # R2, R3: 258 bytes written across the wrap at dist > len (32 768) and dist < len (65 536); a source across the wrap
    add("ring-wrap-258", 254, 259, [("stored", 32600), ("fixed", [lit(68), (258, 1000), lit(1074), (258, 1400), lit(4)]), ("stored", 31174),
                                    ("fixed", [lit(4), (258, 7), lit(3)])], 32)
    # R2, R3: 3 bytes, two before the wrap and one after it, at dist > len and dist < len; a source of 5 bytes across the wrap, repeated
    add("ring-wrap-3", 254, 259, [("stored", 32700), ("fixed", [lit(66), (3, 1000), lit(2), (258, 5), lit(3)]), ("stored", 32400),
                                  ("fixed", [lit(102), (3, 2), lit(3)])], 33)
    # R4: 258 bytes at 32 768 - dist = 1 .. 257 overwrite the slots they have yet to read, in the second window and beyond 65 536
    add("ring-self-overwrite", 272, 249, [("stored", 33000), ("fixed", [it for k in R4_GAPS for it in ((258, WINDOW - k), lit(5))]), ("stored", 31500),
                                          ("fixed", [it for k in (0,) + R4_GAPS for it in ((258, WINDOW - k), lit(5))])], 34)
    # R5, R6: short distances against the turn of 64 lanes; a literal read at once, the second time out of slot 32 767
    add("ring-short-dist", 111, 299, [("fixed", [lit(300)] + [it for d in R5_DISTS for it in ((258, d), lit(3))] +
                                       [(64, 1), lit(3), (65, 1), lit(3), lit(1), (20, 1)]), ("stored", 29634), ("fixed", [lit(68), (258, 1), lit(4)])], 35)
    # R7: dynamic (286 / many distance codes) -> dynamic (258 / one) -> fixed -> stored -> dynamic
    d3 = [lit(300), (258, 1000), lit(2), (40, 2900), lit(2), (7, 3)]
    add("ring-tables", 15, 249, [("dynamic", [lit(2100), (258, 2000), lit(3), (3, 1), lit(2), (10, 30), lit(2), (50, 500), lit(2), (100, 1500), lit(2),
                                             (20, 7), lit(5)]), ("dynamic", [lit(12), (3, 1), lit(5), (3, 1), lit(3), (3, 1)]),
                                 ("fixed", [lit(20), (30, 100), lit(4)]), ("stored", 300), ("dynamic", d3 + [lit(3750 - 2940 - 609)])], 36)
    # R8: Adler-32 where N - i passes through multiples of 65 521
    row = bytes([255]) * 65520
    raw1, raw2 = b"\x01" + row, b"\x01" + row + b"\x02" + row
    out["adler-65521"] = Ring("adler-65521", 1, 65520, [("stored", raw1[:40000]), ("stored", raw1[40000:])], raw1)
    out["adler-131042"] = Ring("adler-131042", 2, 65520, [("stored", raw2[:50000]), ("stored", raw2[50000:100000]), ("stored", raw2[100000:])], raw2)
    return out


def more_valid_files():
    return [("wide-gray-1", simple(3, 1025, 0, 1, None, 41)), ("wide-pal-2", simple(3, 1023, 3, 2, None, 42)), ("wide-gray-4", simple(3, 1023, 0, 4, None, 43)),
            ("paeth-rgba-65x600", simple(65, 600, 6, 8, [4] * 65, 44)),           # rb 2 400: lane 63 runs 63 steps behind across a long row
            ("average-paeth-1000x3", simple(1000, 3, 0, 8, [3, 4] * 500, 45))]     # sixteen bands


# ── errors beyond the first window: the ring files, damaged ─────────────────────────────────────────────────────────────────────────
def _refused(z):
    try:
        zlib.decompress(z)
    except zlib.error:
        return z
    raise AssertionError("zlib accepts a stream meant to be invalid")


@functools.lru_cache(None)
def deep_errors():
    """[(name, file, expected status, raw position at which the decoder meets the error)]"""
    R = ring_files()
    out = []

    def put(name, ring, z, status, pos):
        out.append((name, assemble(ring.H, ring.W, 0, 8, z), status, pos))

    def surplus(ring, blocks, extra):
        return zstream(lambda w: write_blocks(w, blocks), ring.raw[:len(ring.raw) - extra[0]] + extra[1])

    a = R["ring-stored-match"]                                                 # block 3: the stored block of 2 000 bytes from 31 868
    put("deep-cut-in-stored", a, _refused(a.z[:2 + a.marks[3][1] + 1000]), 1, a.block_pos(3) + 1000)
    b = R["ring-self-overwrite"]                                               # block 3, token 0: (258, 32 768) at 66 078; 8 + 5 bits, then 13 extra
    at = token_bitpos(b.blocks, 3, 0) + 13
    put("deep-cut-in-distance-extra", b, _refused(b.z[:2 + at // 8 + 1]), 1, b.block_pos(3))
    c = R["ring-tables"]
    f = [0] * 286
    for s in token_syms(c.blocks[4][1])[0]:
        f[s] += 1
    over = huffman_lengths(f)
    over[over.index(max(over))] -= 1                                           # a complete set with one code shortened
    put("deep-third-header-over-subscribed", c, zbad(lambda w: write_blocks(w, c.blocks, kw={4: {"lit_lens": over}}), c.raw), 2, c.block_pos(4))
    d = R["ring-wrap-258"]
    bad = d.blocks[:1] + [("fixed", d.blocks[1][1] + [("L", 286)])] + d.blocks[2:]
    put("deep-litlen-286", d, zbad(lambda w: write_blocks(w, bad), d.raw), 2, d.block_pos(2))
    far = bytes(np.random.default_rng(8).integers(0, 256, 32767).astype(np.uint8))
    out.append(("distance-32768-at-32767", assemble(182, 183, 0, 8, zbad(lambda w: (stored(w, far), fixed(w, [(258, 32768)], True)))), 3, 32767))
    e = R["ring-wrap-3"]                                                       # cap 66 040; the last block is 500 stored bytes from 65 540
    tail = e.blocks[-1][1]
    put("deep-overflow-literal", b, surplus(b, b.blocks + [("fixed", [7])], (0, b"\x07")), 4, len(b.raw))
    put("deep-overflow-match", e, surplus(e, e.blocks[:-1] + [("stored", tail[:243]), ("fixed", [(258, 9)])], (257, (tail[234:243] * 29)[:258])), 4,
        len(e.raw) - 257)
    put("deep-overflow-stored", e, surplus(e, e.blocks[:-1] + [("stored", tail + b"x")], (0, b"x")), 4, len(e.raw) - 500)
    flip = bytearray(b.z)                                                      # block 2: the stored block of 31 500 bytes from 34 578
    flip[2 + b.marks[2][1] + 65600 - b.block_pos(2)] ^= 0x40
    put("deep-adler-flip", b, _refused(bytes(flip)), 5, 65600)
    # a match that copies a 5 onto the start of row 65: valid deflate, the right Adler-32
    blocks, raw = ring_fill(_pad([("stored", 6450), ("fixed", [("lit", 40), (20, 55), ("lit", 5)])], 7000), 70, 99, 37, force={6500: 5})
    assert match_facts(block_tokens(blocks)) == [(6490, 20, 55)] and raw[6500] == 5 and all(raw[r * 100] <= 4 for r in range(70) if r != 65)
    out.append(("deep-filter-5-by-match", assemble(70, 99, 0, 8, zstream(lambda w: write_blocks(w, blocks), raw)), 7, 6500))
    return out


@functools.lru_cache(None)
def valid_cases():
    """[(name, file)]: every one decodes with status 0"""
    out = []
    for ctype, depth in FORMS:
        for level in (0, 1, 6, 9):
            out.append((f"pillow-{ctype}-{depth}-l{level}", pillow_png(23, 19, ctype, depth, level, level)))
    for ft in range(5):
        out.append((f"filter-{ft}", simple(9, 17, 2, 8, [ft] * 9, ft)))
        out.append((f"filter-{ft}-pal4", simple(9, 17, 3, 4, [ft] * 9, ft)))
    out.append(("filters-mixed", simple(11, 13, 6, 8, None, 5)))
    out.append(("filters-mixed-la", simple(11, 13, 4, 8, None, 6)))
    out.append(("idat-1-byte", simple(5, 7, 2, 8, None, 1, idat=1)))              # every Huffman code is cut by a chunk boundary
    out.append(("idat-0-bytes", simple(5, 7, 0, 8, None, 2, idat=0)))
    out.append(("idat-cut-3", simple(9, 17, 2, 8, None, 3, smooth=True, cuts=[3, 40])))
    out.append(("ancillary", simple(4, 6, 3, 2, None, 4, extra=[chunk(b"gAMA", struct.pack(">I", 45455)), chunk(b"tEXt", b"k\0v")],
                                    after=[chunk(b"tIME", bytes(7))])))
    out.append(("no-iend", simple(4, 6, 0, 4, None, 4, end=False)))
    W, H = 20, 4
    raw = bytearray(np.random.default_rng(3).integers(0, 256, H * (W + 1)).astype(np.uint8))
    for r in range(H):
        raw[r * (W + 1)] = (r + 1) % 5
    raw = bytes(raw)
    lits = list(raw)
    out.append(("stored-empty-first", gray_file(H, W, lambda w: (stored(w, b""), fixed(w, lits, True)), raw)))
    out.append(("stored-split", gray_file(H, W, lambda w: (stored(w, raw[:30]), stored(w, b""), stored(w, raw[30:], True)), raw)))
    out.append(("fixed", gray_file(H, W, lambda w: fixed(w, lits, True), raw)))
    out.append(("fixed-fixed-off-grid", gray_file(H, W, lambda w: (fixed(w, lits[:11]), fixed(w, lits[11:], True)), raw)))   # the second header starts inside a byte
    out.append(("dynamic", gray_file(H, W, lambda w: dynamic(w, lits, True), raw)))
    out.append(("dynamic-no-repeats", gray_file(H, W, lambda w: dynamic(w, lits, True, repeats=False), raw)))
    out.append(("fixed-dynamic-stored", gray_file(H, W, lambda w: (fixed(w, lits[:5]), dynamic(w, lits[5:50]), stored(w, raw[50:], True)), raw)))
    # a 15-bit code: lengths 1, 2, ..., 14, 15, 15 over sixteen symbols is complete
    W2, H2 = 31, 2
    lens15 = [0] * 286
    for i, s in enumerate([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 256]):
        lens15[s] = i + 1
    lens15[200] = lens15[201] = 15
    raw2 = bytearray([1] + [1 + i % 13 for i in range(W2)] + [2] + [1 + (3 * i) % 13 for i in range(W2)])   # (filter types 1 and 2)
    raw2[5], raw2[40] = 200, 201
    raw2 = bytes(raw2)
    out.append(("dynamic-15-bit-code", gray_file(H2, W2, lambda w: dynamic(w, list(raw2), True, lit_lens=lens15), raw2)))
    # matches: length 3, length 258, distance 1 (a run), distance < length; one distance code (an incomplete set zlib accepts)
    W3, H3 = 299, 2
    row = [0] + [9, 8, 7] + [9, 8, 7] + [5] * 258 + [1, 2, 3, 4, 5, 6, 7] * 5
    raw3 = bytes(row + [1] + row[1:])
    t3 = [0, 9, 8, 7, (3, 3), 5, (257, 1), 1, 2, 3, 4, 5, 6, 7, (28, 7), 1] + [(258, 300), (41, 300)]
    out.append(("matches", gray_file(H3, W3, lambda w: fixed(w, t3, True), raw3)))
    out.append(("matches-dynamic", gray_file(H3, W3, lambda w: dynamic(w, t3, True), raw3)))
    raw4 = bytes([0] + [6] * W + [2] + [0] * W + [0] + [6] * W + [1] + [0] * W)
    t4 = [0, 6, (W - 1, 1), 2, 0, (W - 1, 1), (W + 1, 2 * (W + 1)), 1, 0, (W - 1, 1)]
    out.append(("one-distance-code", gray_file(H, W, lambda w: dynamic(w, [0, 6, (W - 1, 1), 2, 0, (W - 1, 1), 0, 6, (W - 1, 1), 1, 0, (W - 1, 1)], True), raw4)))
    out.append(("two-distance-codes", gray_file(H, W, lambda w: dynamic(w, t4, True), raw4)))
    big = bytes([0]) + bytes(np.random.default_rng(9).integers(0, 256, 65534).astype(np.uint8))
    out.append(("stored-65535", assemble(1, 65534, 0, 8, zstream(lambda w: (stored(w, big), stored(w, b"", True)), big))))
    out.append(("far-match-32768", far_match_file()))
    out += [(n, r.file) for n, r in ring_files().items()] + more_valid_files()
    return out


# ── the hostile corpus ──────────────────────────────────────────────────────────────────────────────────────────────────────────────
def with_stream(png, z):
    """the file with its IDAT chunks replaced by one that holds z (CRCs recomputed)"""
    cs = chunks_of(png)
    out, done = SIG, False
    for t, d in cs:
        if t == b"IDAT":
            if not done:
                out += chunk(b"IDAT", z)
                done = True
        else:
            out += chunk(t, d)
    return out


def stream_of(png):
    return b"".join(d for t, d in chunks_of(png) if t == b"IDAT")


@functools.lru_cache(None)
def hand_made_invalid():
    """[(name, file, expected status or None)]: 17 x 9 RGB files around streams zlib refuses, files the parser refuses, and the ring
    files damaged beyond the first window (deep_errors)"""
    H, W = 9, 17
    rows = rng_rows(H, W, 2, 8, 11)
    raw = filter_rows(rows, [r % 5 for r in range(H)], 3)
    lits = list(raw)
    good = canon(FIXED_LIT)
    mk = lambda z: assemble(H, W, 2, 8, z)   # noqa: E731
    out = []

    def bad(name, build, status, **kw):
        out.append((name, mk(zbad(build, raw, **kw)), status))

    bad("block-type-3", lambda w: (w.put(1, 1), w.put(3, 2)), 2)
    bad("len-nlen", lambda w: stored(w, raw, True, nlen=0x1234), 2)
    over = [0] * 286
    over[0] = over[1] = over[256] = 1
    bad("litlen-over-subscribed", lambda w: dynamic(w, [0, 1], True, lit_lens=over), 2)
    inc = [0] * 286
    inc[0] = inc[256] = 2
    bad("litlen-incomplete", lambda w: dynamic(w, [0, 0], True, lit_lens=inc), 2)
    two = [0] * 30
    two[0] = two[1] = two[2] = 2
    bad("distance-incomplete", lambda w: dynamic(w, [1, 1, (3, 1), (3, 2)], True, dist_lens=two), 2)
    cl = [0] * 19
    cl[16] = cl[0] = 1
    bad("repeat-without-previous", lambda w: dynamic(w, [], True, cl_seq=[(16, 0)] + [(0, 0)] * 300, cl_lens=cl), 2)
    cl2 = [0] * 19
    cl2[18] = cl2[1] = 1
    bad("repeat-past-the-end", lambda w: dynamic(w, [], True, cl_seq=[(1, 0)] + [(18, 127)] * 3, cl_lens=cl2, hlit=257, hdist=1), 2)
    noeob = [8] * 256 + [0] * 30
    bad("no-end-of-block-code", lambda w: dynamic(w, [1, 2], True, lit_lens=noeob, eob=False), 2)
    bad("code-length-code-incomplete", lambda w: dynamic(w, [1], True, cl_lens=[0, 3, 0, 0, 0, 0, 0, 0, 3] + [0] * 10,
                                                           cl_seq=[(8, 0)] * 257 + [(1, 0)]), 2)
    bad("hlit-287", lambda w: dynamic(w, [1], True, lit_lens=[8] * 286, hlit=287), 2)
    bad("litlen-286", lambda w: fixed(w, lits[:5] + [("L", 286)], True), 2)
    bad("distance-30", lambda w: fixed(w, lits[:5] + [("D", 3, 30)], True), 2)
    bad("all-zero-distance-set-used", lambda w: dynamic(w, [1, 1, 1, ("L", 257)], True, dist_lens=[0]), 2)
    bad("distance-before-start", lambda w: fixed(w, lits[:4] + [(3, 5)] + lits[7:], True), 3)
    bad("distance-at-position-0", lambda w: fixed(w, [(3, 1)] + lits[3:], True), 3)
    w = Bits()
    fixed(w, lits, False)
    cut = b"\x78\x9c" + w.bytes()                              # the bytes end behind a block that is not the last
    try:
        zlib.decompress(cut)
        raise AssertionError("zlib accepts a stream without a final block")
    except zlib.error:
        out.append(("truncated-no-final-block", mk(cut), 1))
    bad("cm-7", lambda w: fixed(w, lits, True), 5, header=b"\x77\x85")
    bad("fdict", lambda w: fixed(w, lits, True), 5, header=b"\x78\xbb")
    bad("fcheck", lambda w: fixed(w, lits, True), 5, header=b"\x78\x9d")
    bad("cinfo-8", lambda w: fixed(w, lits, True), 5, header=b"\x88\x1c")
    bad("adler", lambda w: fixed(w, lits, True), 5, adler=zlib.adler32(raw) ^ 0x10000)
    # streams zlib accepts but the file's size does not
    out.append(("output-overflow-literal", mk(zstream(lambda w: fixed(w, lits + [7], True), raw + b"\x07")), 4))
    out.append(("output-overflow-match", mk(zstream(lambda w: fixed(w, lits + [(9, 4)], True), raw + (raw[-4:] * 3)[:9])), 4))
    out.append(("output-overflow-stored", mk(zstream(lambda w: stored(w, raw + b"ab", True), raw + b"ab")), 4))
    out.append(("short-by-a-row", mk(zlib.compress(raw[:-(1 + 3 * W)])), 1))
    out.append(("trailer-cut", mk(zlib.compress(raw)[:-2]), 1))
    b5 = bytearray(raw)
    b5[3 * (1 + 3 * W)] = 5
    out.append(("filter-type-5", mk(zlib.compress(bytes(b5))), 7))
    b9 = bytearray(raw)
    b9[0] = 255
    out.append(("filter-type-255", mk(zlib.compress(bytes(b9))), 7))
    # the parser's refusals
    ok = mk(zlib.compress(raw))
    z = zlib.compress(raw)
    ihdr = lambda **k: struct.pack(">IIBBBBB", k.get("W", W), k.get("H", H), k.get("depth", 8), k.get("ctype", 2), k.get("comp", 0),   # noqa: E731
                                   k.get("filt", 0), k.get("lace", 0))
    refuse = [("sixteen-bit", assemble(H, W, 2, 16, z)), ("adam7", assemble(H, W, 2, 8, z, interlace=1)), ("rgb-at-4", assemble(H, W, 2, 4, z)),
              ("type-5", assemble(H, W, 5, 8, z)), ("palette-16", assemble(H, W, 3, 16, z, plte=palette(4))),
              ("compression-1", assemble(H, W, 2, 8, z, ihdr=ihdr(comp=1))), ("filter-method-1", assemble(H, W, 2, 8, z, ihdr=ihdr(filt=1))),
              ("bad-crc", ok[:40] + bytes([ok[40] ^ 1]) + ok[41:]), ("bad-crc-ihdr", ok[:29] + bytes([ok[29] ^ 1]) + ok[30:]),
              ("chunk-leaves-the-file", ok[:60]), ("missing-plte", assemble(H, W, 3, 8, z)), ("plte-of-4-bytes", assemble(H, W, 3, 8, z, plte=bytes(4))),
              ("plte-of-771-bytes", assemble(H, W, 3, 8, z, plte=bytes(771))), ("H-0", assemble(0, W, 2, 8, z)), ("W-0", assemble(H, 0, 2, 8, z)),
              ("too-many-pixels", assemble(4097, 4096, 0, 8, z)), ("no-idat", SIG + chunk(b"IHDR", ihdr()) + chunk(b"IEND", b"")),
              ("no-signature", b"\x89PNG\r\n\x1a\r" + ok[8:]), ("ihdr-second", SIG + chunk(b"gAMA", bytes(4)) + ok[8:]),
              ("ihdr-of-12-bytes", SIG + chunk(b"IHDR", ihdr()[:12]) + ok[33:]), ("empty", b""), ("signature-only", SIG),
              ("critical-unknown", ok[:33] + chunk(b"ABCD", b"xy") + ok[33:])]
    out += [(n, f, 6) for n, f in refuse]
    out += [(n, f, s) for n, f, s, _ in deep_errors()]
    return out


def _mutants(png):
    """the file cut at every byte, and every bit of its zlib stream flipped with the CRC recomputed"""
    out = [png[:n] for n in range(len(png))]
    z = stream_of(png)
    for i in range(8 * len(z)):
        m = bytearray(z)
        m[i >> 3] ^= 1 << (i & 7)
        out.append(with_stream(png, bytes(m)))
    return out


@functools.lru_cache(None)
def hostile_corpus():
    """[file]: the mutants of a 17 x 9 RGB file and of its 4-bit palette twin, then the hand-made files (the deep errors last)"""
    H, W = 9, 17
    rgb = simple(H, W, 2, 8, None, 21, smooth=True)
    pal = simple(H, W, 3, 4, None, 22, plte=palette(11, 3))
    return _mutants(rgb) + _mutants(pal) + [f for _, f, _ in hand_made_invalid()]


def corpus_blob(files):
    return struct.pack("<I", len(files)) + b"".join(struct.pack("<I", len(f)) + f for f in files)
