"""Inputs of the JPEG decoder's tests (helper module, like tests/mjpeg_cases.py): Pillow-encoded files of seeded noise in every accepted
form, and the hostile corpus -- truncations, single-byte substitutions and damaged restart markers of two small 4:2:0 files -- that
tests/test_mjpd_host.py holds the twin to, tools/mjpd_host_fuzz.cpp runs under sanitizers, and tests/test_gpu_mjpd.py takes its
status cases from; the Annex-K scan writer for hand-made gray files (`Scan`, and `RstScan` for scans with restart markers); and the
files that place what the twin does not share with the device -- restart markers on the edges of k_mjpd_markers' strides and waves,
frames across k_mjpd_entropy's workgroups, narrow planes, long codes, values past the int32 bound -- each builder asserting on the
bytes what it is named for.  Everything is cached: a file is encoded once per process."""
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


# ── the scan writer: hand-made gray scans in the Annex K luminance tables (tests/mjps_cases.py uses it too) ───────────────────────────
@functools.lru_cache(maxsize=None)
def _dht(jpeg):
    """`{(class, id): {symbol: (code, length)}}` of a file's DHT segments."""
    tabs, at = {}, 2
    while jpeg[at + 1] != 0xDA:
        n = 2 + ((jpeg[at + 2] << 8) | jpeg[at + 3])
        if jpeg[at + 1] == 0xC4:
            s, i = jpeg[at + 4:at + n], 0
            while i < len(s):
                tc, th = s[i] >> 4, s[i] & 15
                counts = s[i + 1:i + 17]
                vals = s[i + 17:i + 17 + sum(counts)]
                code, k, t = 0, 0, {}
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        t[vals[k]] = (code, length)
                        code += 1
                        k += 1
                    code <<= 1
                tabs[(tc, th)] = t
                i += 17 + sum(counts)
        at += n
    return tabs


def pack_bits(bits):
    """Bits -> the bytes of a scan: padded with 1-bits to a whole byte, a 00 stuffed behind every FF."""
    a = np.asarray(bits, np.uint8)
    a = np.concatenate([a, np.ones(-a.size % 8, np.uint8)])
    return np.packbits(a).tobytes().replace(b"\xff", b"\xff\x00")


class Scan:
    """A gray scan bit by bit, in the Annex K luminance tables (taken from a Pillow file, which carries them)."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.head = pillow_jpeg(H, W, "gray", 75, 0)
        self.dc_tab, self.ac_tab = _dht(self.head)[(0, 0)], _dht(self.head)[(1, 0)]
        self.blocks = ((H + 7) // 8) * ((W + 7) // 8)
        self.bits = []

    def raw(self, bits):
        self.bits += [int(b) for b in bits]
        return self

    def _code(self, table, sym):
        code, length = table[sym]
        return self.raw(format(code, f"0{length}b"))

    def _value(self, v):
        size = int(abs(v)).bit_length()
        if size:
            self.raw(format(v if v > 0 else v + (1 << size) - 1, f"0{size}b"))
        return size

    def dc(self, diff):
        self._code(self.dc_tab, int(abs(diff)).bit_length())
        self._value(diff)
        return self

    def ac(self, run, v):
        self._code(self.ac_tab, (run << 4) | int(abs(v)).bit_length())
        self._value(v)
        return self

    def zrl(self):
        return self._code(self.ac_tab, 0xF0)

    def eob(self):
        return self._code(self.ac_tab, 0x00)

    def block(self, diff, ac=()):
        """One block from its DC difference and `{zigzag index: value}`."""
        self.dc(diff)
        ac = dict(ac)
        at = 1
        for k in sorted(ac):
            run = k - at
            while run > 15:
                self.zrl()
                run -= 16
            self.ac(run, ac[k])
            at = k + 1
        return self.eob() if at < 64 else self

    def scan_bytes(self):
        return pack_bits(self.bits)

    def file(self, tail=b""):
        lo, _ = scan_span(self.head)
        return self.head[:lo] + self.scan_bytes() + tail + b"\xff\xd9"


# ── restart scans: where k_mjpd_markers' 256-byte strides and 64-byte wave slices meet the RSTm ───────────────────────────────────────
# k_mjpd_markers walks a scan 256 bytes at a time, a byte per lane, four waves of 64: a marker whose FF is byte i of the scan lies in
# stride i // 256 and wave slice (i % 256) // 64, and it is numbered from the markers before it in the scan.  What follows builds
# files whose markers lie where that numbering is decided, and every builder asserts its placement on the bytes it returns.
STRIDE, SLICE = 256, 64


class RstScan:
    """A gray scan of restart intervals: each interval a `Scan` bit list (the DC prediction starts at 0 in each), padded and stuffed
    on its own, the intervals joined by FF D0+number(k).  The head is Pillow's file with the same Ri: DRI and tables are its own."""

    def __init__(self, H, W, Ri):
        self.H, self.W, self.Ri = H, W, Ri
        self.head = pillow_jpeg(H, W, "gray", 75, Ri)
        self.blocks = ((H + 7) // 8) * ((W + 7) // 8)
        self.nI = -(-self.blocks // Ri)
        assert _dht(self.head) == _dht(pillow_jpeg(H, W, "gray", 75, 0))
        self.intervals = []

    def interval(self):
        """The next interval, to be written block by block."""
        self.intervals.append(Scan(self.H, self.W))
        return self.intervals[-1]

    def scan_bytes(self, number=lambda k: k & 7):
        parts = [self.intervals[0].scan_bytes()]
        for k, s in enumerate(self.intervals[1:]):
            parts += [bytes([0xFF, 0xD0 + number(k)]), s.scan_bytes()]
        return b"".join(parts)

    def file(self, number=lambda k: k & 7, tail=b""):
        lo, _ = scan_span(self.head)
        return self.head[:lo] + self.scan_bytes(number) + tail + b"\xff\xd9"


def marker_offsets(jpeg):
    """The offset of every RSTm's FF inside the scan."""
    lo, _ = scan_span(jpeg)
    return [i - lo for i in rst_positions(jpeg)]


def scan_length(jpeg):
    lo, hi = scan_span(jpeg)
    return hi - lo


def _acs(rng, nac, amp=40):
    """`{zigzag index: value}` of `nac` non-zero AC values up to `amp` in magnitude."""
    ks = rng.choice(np.arange(1, 64), nac, replace=False)
    return {int(k): int(rng.integers(1, amp + 1)) * (1 if rng.integers(2) else -1) for k in ks}


def _dense_scan(seed):
    s = RstScan(8, 2400, 1)
    rng = np.random.default_rng([8, 2400, seed])
    for _ in range(s.nI):
        s.interval().block(int(rng.integers(-3, 4)))
    return s


def per_slice(jpeg):
    """`{(stride, wave slice): markers whose FF lies in it}`."""
    out = {}
    for i in marker_offsets(jpeg):
        key = (i // STRIDE, i % STRIDE // SLICE)
        out[key] = out.get(key, 0) + 1
    return out


@functools.lru_cache(maxsize=None)
def dense(seed=0):
    """8 x 2400 gray, Ri = 1: 300 intervals of one block (a DC difference of -3..3 and EOB: one or two bytes), so a wave's ballot holds
    many markers, every wave of a stride has some, and the count passes 255 and wraps k & 7 thirty-seven times."""
    j = _dense_scan(seed).file()
    slices = per_slice(j)
    assert MJ.parse(j)["nI"] == 300 and len(marker_offsets(j)) == 299 > 255
    assert max(slices.values()) >= 8                                                       # several markers in one wave
    assert any(all((s, w) in slices for w in range(4)) for s in range(scan_length(j) // STRIDE))   # all four waves of a stride
    assert scan_length(j) > 4 * STRIDE
    return j


def empty_strides(jpeg):
    """Whole strides of the scan without a marker's FF that a later stride with one follows."""
    at = {i // STRIDE for i in marker_offsets(jpeg)}
    return [s for s in range(max(at)) if s not in at]


def empty_slices(jpeg):
    at = set(per_slice(jpeg))
    last = max(at)
    return [(s, w) for s in range(last[0] + 1) for w in range(4) if (s, w) not in at and (s, w) < last]


SPARSE_SHAPE = (8, 400, 10)     # 50 blocks, 5 intervals of 10 blocks of 60 small AC values: above 256 bytes each


@functools.lru_cache(maxsize=None)
def sparse(seed=0):
    """Intervals longer than a stride: whole strides and wave slices without a marker between those that have one, so the running
    `base` is carried over strides that add nothing to it."""
    H, W, Ri = SPARSE_SHAPE
    s = RstScan(H, W, Ri)
    rng = np.random.default_rng([H, W, Ri, seed])
    for k in range(s.nI):
        iv = s.interval()
        for _ in range(min(Ri, s.blocks - k * Ri)):
            iv.block(int(rng.integers(-3, 4)), _acs(rng, 60, 4))      # (small values: inside the bound, where the twin is Pillow)
    j = s.file()
    off = marker_offsets(j)
    assert len(off) == s.nI - 1 == 4 and all(b - a > STRIDE for a, b in zip([0] + off, off + [scan_length(j)]))
    assert empty_strides(j) and empty_slices(j)
    return j


EDGE_SHAPE = (8, 96)            # 12 blocks, Ri = 1: eleven markers


@functools.lru_cache(maxsize=None)
def edge_file(seed):
    """8 x 96 gray, Ri = 1, every block with 0..49 random AC values: the family the placements below are searched in."""
    H, W = EDGE_SHAPE
    s = RstScan(H, W, 1)
    rng = np.random.default_rng([H, W, seed])
    for _ in range(s.nI):
        s.interval().block(int(rng.integers(-3, 4)), _acs(rng, int(rng.integers(0, 50))))
    return s.file()


def residues(jpeg):
    """Offsets mod 256 of the markers' FFs.  255: the marker straddles two strides (its FF is the last lane's byte, its number the
    next stride's first); 254: the last whole marker of a stride; 0: the first; 63 and 64: across and behind a wave's edge."""
    return {i % STRIDE for i in marker_offsets(jpeg)}


# residue set -> the seeds of edge_file whose markers hold all of it (the first two of a search over seeds 0..2000), pinned
EDGES = {(255,): (15, 19), (254,): (150, 163), (0,): (24, 44), (63, 64): (1193, 1836), (0, 255): (198, 1521)}
# scan_length % 256 -> seed: the kernel's tail test is i + 1 < n
LENGTHS = {0: 527, 1: 610, 255: 60}


def search_edges(seeds=range(2001)):
    """What pinned EDGES and LENGTHS: `({residue set: [seeds]}, {length residue: [seeds]})`, each list the first two that fire."""
    edges, lengths = {R: [] for R in EDGES}, {r: [] for r in LENGTHS}
    for seed in seeds:
        j = edge_file(seed)
        if not np.array_equal(twin(j)[0], pillow_bgr(j)):      # (49 values of up to 40 can leave the header's bound: no parity is claimed there)
            continue
        res = residues(j)
        for R, found in edges.items():
            if len(found) < 2 and set(R) <= res:
                found.append(seed)
        r = scan_length(j) % STRIDE
        if r in lengths and len(lengths[r]) < 2:
            lengths[r].append(seed)
    return edges, lengths


def edge_case(R, which=0):
    j = edge_file(EDGES[R][which])
    assert set(R) <= residues(j), (R, which, sorted(residues(j)))
    assert len(marker_offsets(j)) == 11
    return j


def length_case(r):
    j = edge_file(LENGTHS[r])
    assert scan_length(j) % STRIDE == r and scan_length(j) > STRIDE, (r, scan_length(j))
    return j


def valid_placements():
    """`[(label, file)]`: every placement file that is a valid JPEG (twin status 0, and Pillow's bytes)."""
    out = [("dense", dense(0)), ("dense'", dense(1)), ("sparse", sparse(0)), ("sparse'", sparse(1))]
    out += [(f"edge-{R}-{w}", edge_case(R, w)) for R in EDGES for w in (0, 1)]
    return out + [(f"length-{r}", length_case(r)) for r in LENGTHS]


@functools.lru_cache(maxsize=None)
def damaged():
    """`{name: (file, the twin's status)}`: dense(0) with its markers damaged away from stride 0 and wave 0, where the thin cases
    of the hostile corpus never reach.  Each asserts on its bytes what it is named for."""
    s, j = _dense_scan(0), dense(0)
    lo, hi = scan_span(j)
    pos = rst_positions(j)
    out = {}
    late = s.file(number=lambda k: (k + 1) & 7 if k == 200 else k & 7)
    assert [a != b for a, b in zip(late, j)].count(True) == 1 and late[pos[200] + 1] != j[pos[200] + 1] and pos[200] - lo >= STRIDE
    out["renumbered-late"] = (late, 5)
    by4 = s.file(number=lambda k: (k + 4) & 7 if k == 201 else k & 7)      # right modulo 4: only a comparison of all three bits sees it
    assert [a != b for a, b in zip(by4, j)].count(True) == 1 and by4[pos[201] + 1] ^ j[pos[201] + 1] == 4
    out["renumbered-by-4"] = (by4, 5)
    mod7 = s.file(number=lambda k: k % 7 if k >= 8 else k)
    assert len(mod7) == len(j) and min(i for i in range(len(j)) if mod7[i] != j[i]) == pos[8] + 1      # the first eight markers are right:
    assert [mod7[p + 1] for p in pos[:9]] == [0xD0 + k for k in range(8)] + [0xD1] and j[pos[8] + 1] == 0xD0   # only the wrap is wrong
    out["mod7"] = (mod7, 5)
    removed = j[:pos[-1]] + j[pos[-1] + 2:]
    assert len(rst_positions(removed)) == 298 and rst_positions(removed) == pos[:-1]
    out["removed-last"] = (removed, 5)
    doubled = bytearray(j[:lo])
    at = lo
    for p in pos:
        doubled += j[at:p + 2] + j[p:p + 2]
        at = p + 2
    doubled = bytes(doubled + j[at:])
    assert len(rst_positions(doubled)) == 2 * 299 and len(doubled) == len(j) + 2 * 299       # 598 markers for 299 places
    out["doubled-all"] = (doubled, 5)
    end = s.file(tail=b"\xff\xd3")
    n = scan_length(end)
    assert marker_offsets(end)[-1] == n - 2 and len(marker_offsets(end)) == 300 and end[-4:] == b"\xff\xd3\xff\xd9"
    out["end-marker"] = (end, 5)
    ff = j[:-1]
    assert ff[-1] == 0xFF and ff[-2] != 0xFF and scan_length(ff) == scan_length(j) + 1 and len(rst_positions(ff)) == 299
    out["ff-last"] = (ff, 0)
    return out


GUARD_ORDER = ("dense", "doubled-all", "dense'", "renumbered-late", "dense", "doubled-all")
GUARD_STATUS = [0, 5, 0, 5, 0, 5]


def guard_batch():
    """The neighbour order that makes the write guard k + 1 < nI observable: a frame of 598 markers before a good frame's interval
    table, and as the call's last frame before the statuses."""
    d = damaged()
    return [dense(0) if n == "dense" else dense(1) if n == "dense'" else d[n][0] for n in GUARD_ORDER]


# ── the entropy pass's lane map: lane i = interval i % nI of frame i // nI, 64 lanes per workgroup ───────────────────────────────────
LANE_Q = (30, 95, 75, 50, 100, 60, 85)


@functools.lru_cache(maxsize=None)
def lane_files():
    """Seven distinct 37 x 50 4:2:0 files with per-file tables, Ri = 1, nI = 12: 84 lanes, so the second workgroup starts at frame 5,
    interval 4."""
    files = tuple(pillow_jpeg(37, 50, "420", q, 1, True, seed) for seed, q in enumerate(LANE_Q))
    assert all(MJ.parse(j)["nI"] == 12 for j in files) and 64 // 12 == 5 and 64 % 12 == 4
    assert MJ.records_host(list(files))[3].shape[0] == 7
    assert len({twin(j)[0].tobytes() for j in files}) == 7
    return files


def rst_removed(jpeg, which=0):
    """The file without one of its RSTm."""
    p = rst_positions(jpeg)[which]
    return jpeg[:p] + jpeg[p + 2:]


@functools.lru_cache(maxsize=None)
def lane_batch(nI):
    """`(files, lane 64's (frame, interval))` of a call at an nI that does not divide 64, in which a workgroup boundary falls inside
    a frame.  nI = 20 (4:2:2, Ri = 1): four distinct frames, 80 lanes.  nI = 3 (4:2:0, Ri = 5): six distinct files; 18 lanes would
    stay inside one workgroup, so the six are dealt out over 24 frames, 72 lanes, in four different orders -- no two neighbours are
    equal, and no frame equals the one six places on, which a fixed cycle would allow."""
    if nI == 20:
        files = [pillow_jpeg(37, 50, "422", q, 1, True, seed) for seed, q in enumerate(LANE_Q[:4])]
    else:
        assert nI == 3
        six = [pillow_jpeg(37, 50, "420", q, 5, True, seed) for seed, q in enumerate(LANE_Q[:6])]
        order = [0, 1, 2, 3, 4, 5, 2, 0, 4, 1, 5, 3, 1, 3, 0, 5, 2, 4, 3, 2, 5, 0, 4, 1]
        assert all(sorted(order[k:k + 6]) == list(range(6)) for k in range(0, 24, 6)) and all(order[k] != order[k + 6] for k in range(18))
        files = [six[k] for k in order]
    assert all(MJ.parse(j)["nI"] == nI for j in files) and 64 % nI and len(files) * nI > 64
    assert len({twin(j)[0].tobytes() for j in files}) == (4 if nI == 20 else 6)
    assert all(twin(a)[0].tobytes() != twin(b)[0].tobytes() for a, b in zip(files, files[1:]))
    return files, (64 // nI, 64 % nI)


# ── narrow planes: chroma of one or two columns is replicated (og_jpegd_chroma's cw <= 2), a 1 x 1 frame has 8..24 live idct lanes ────
NARROW = tuple((H, W, form) for H, W in ((2, 3), (3, 4), (5, 5), (4, 6), (3, 2), (16, 1)) for form in ("422", "420")) + \
         tuple((1, 1, form) for form in FORMS)


def narrow_files(H, W, form):
    """Three distinct seeds of one narrow shape (quality 90, as tests/test_mjpd_host.py's replication test)."""
    return [pillow_jpeg(H, W, form, 90, 0, False, seed) for seed in range(3)]


# ── long codes ───────────────────────────────────────────────────────────────────────────────────────────────────────────────────────
def long_lengths(table):
    """The code lengths of 9 bits and more that a `_dht` table has."""
    return sorted({length for _, length in table.values() if length >= 9})


@functools.lru_cache(maxsize=None)
def long_codes():
    """`(file, lengths)`: gray 8 x 64, its blocks holding, for each length of 9 bits and more in the luminance AC table, the run/size
    symbol of that length with the smallest size (then run); positive values in odd blocks, negative in even ones.  9 bits is the
    last length of the 512-entry look-up; from 10 on og_jpegd_symbol walks maxcode/valoff/vals."""
    s = Scan(8, 64)
    lengths = long_lengths(s.ac_tab)
    assert lengths[0] == 9 and lengths[-1] == 16 and len(lengths) >= 4
    picks = []
    for length in lengths:
        sym = min((sym for sym, (_, n) in s.ac_tab.items() if n == length and sym & 15), key=lambda v: (v & 15, v >> 4))
        picks.append((sym >> 4, sym & 15))
    groups = [[]]                                     # the symbols of small sizes have long runs: as many to a block as its 63 places take
    for run, size in picks:
        if sum(r + 1 for r, _ in groups[-1]) + run + 1 > 63:
            groups.append([])
        groups[-1].append((run, size))
    assert 2 * len(groups) <= s.blocks and sum(map(len, groups)) == len(lengths)
    for b in range(s.blocks):                         # blocks 2 g and 2 g + 1 hold group g: each symbol with a negative and a positive value
        ac, k = {}, 0
        for run, size in groups[(b // 2) % len(groups)]:
            k += run + 1
            ac[k] = (1 << (size - 1)) * (1 if b & 1 else -1)
        s.block((b % 7) - 3, ac)
    return s.file(), tuple(lengths)


@functools.lru_cache(maxsize=None)
def long_chroma():
    """A 4:4:4 Pillow file with `optimize=True` whose own chroma tables hold codes above 9 bits."""
    j = pillow_jpeg(37, 50, "444", 95, 0, True, 3)
    t = _dht(j)
    assert max(long_lengths(t[(1, 1)])) > 9 and MJ.parse(j)["sampling"] == 1
    return j


# ── past the int32 bound ─────────────────────────────────────────────────────────────────────────────────────────────────────────────
def _handmade_gray(dc, q):
    """An 8x8 gray file of ONE coefficient: DC = dc, every quantisation step q."""
    codes = {0: "00", 1: "010", 2: "011", 3: "100", 4: "101", 5: "110", 6: "1110", 7: "11110", 8: "111110", 9: "1111110", 10: "11111110",
             11: "111111110"}                                             # Annex K.3, luminance DC
    j = bytearray(pillow_jpeg(8, 8, "gray"))
    at = j.index(b"\xff\xdb")
    j[at + 5:at + 69] = bytes([q]) * 64
    lo, _ = scan_span(bytes(j))
    cat = abs(dc).bit_length()
    bits = codes[cat] + (format(dc if dc >= 0 else dc + (1 << cat) - 1, f"0{cat}b") if cat else "") + "1010"      # EOB
    bits += "1" * (-len(bits) % 8)
    scan = bytes(int(bits[k:k + 8], 2) for k in range(0, len(bits), 8)).replace(b"\xff", b"\xff\x00")
    return bytes(j[:lo]) + scan + b"\xff\xd9"


PAST_DC = (2047, 0, -2047, -1023, 1023, 2047, 0, -2047)


@functools.lru_cache(maxsize=None)
def past_the_bound():
    """Gray 8 x 64, every quantisation step 255, the DC predictions PAST_DC (every difference inside category 11) and all 63 AC values
    +-1023: a block's dequantised norm is some 2 000 000 against the bound's 5 900, so every pass of og_jpegd_idct8 wraps."""
    s = Scan(8, 64)
    rng = np.random.default_rng(1023)
    pred = 0
    for dc in PAST_DC:
        assert abs(dc - pred) <= 2047
        s.block(dc - pred, {k: 1023 if rng.integers(2) else -1023 for k in range(1, 64)})
        pred = dc
    j = bytearray(s.file())
    at = j.index(b"\xff\xdb")
    assert j[at + 2:at + 5] == b"\x00\x43\x00"
    j[at + 5:at + 69] = bytes([255]) * 64
    return bytes(j)
