"""Inputs of the split entropy decoder's tests (helper module beside tests/mjpd_cases.py, whose Pillow files and hostile corpus it
reuses): the (sub, lanes) pairs of the issue, a second hostile corpus from a 37x50 4:2:0 file without DRI, and a small Annex-K scan
writer for hand-made gray files -- coefficient blocks and raw bits in, bytes out -- whose claimed statuses the sequential twin
confirms.  Everything is cached."""
import functools

import numpy as np

import mjpd_cases as DC
from openglottal_amd import mjpeg as MJ

PAIRS = ((4, 2), (4, 256), (8, 3), (64, 256), (1024, 256))      # (sub, lanes per window)
SMALL = ((4, 2), (4, 256))


def split(jpeg, sub, lanes, stats=False):
    return MJ.decode_split_host(jpeg, sub, lanes, statuses=True, stats=stats)


def same_as_twin(jpeg, pairs=PAIRS):
    """Holds the split twin to the sequential one on one file; returns the status."""
    ref, st = DC.twin(jpeg)
    for sub, lanes in pairs:
        out, st2 = split(jpeg, sub, lanes)
        assert st2 == st, (sub, lanes, st, st2)
        if ref is None:
            assert out is None
        else:
            assert int(np.abs(out.astype(np.int16) - ref).max()) == 0, (sub, lanes)
    return st


@functools.lru_cache(maxsize=None)
def base37():
    """37x50 4:2:0 without DRI: several hundred bytes."""
    j = DC.pillow_jpeg(37, 50, "420", 30, 0)
    assert 300 < len(j) < 2000 and MJ.parse(j)["Ri"] == 0
    return j


def corpus_of(j, name):
    out = [(f"{name}-cut{n}", j[:n]) for n in range(len(j))]
    lo, hi = DC.scan_span(j)
    rng = np.random.default_rng(len(j))
    for k in range(500):
        b = bytearray(j)
        at = int(rng.integers(lo, hi))
        b[at] = int(rng.integers(0, 256))
        out.append((f"{name}-sub{k}@{at}", bytes(b)))
    return out


@functools.lru_cache(maxsize=None)
def hostile():
    """`[(label, bytes)]`: every truncation and the 500 substitutions of mjpd_cases.bases()[1] (as mjpd_cases.hostile makes them),
    and the same made from base37()."""
    first = [(label, b) for label, b in DC.hostile() if label.startswith("nodri-")]
    assert len(first) == len(DC.bases()[1]) + 500
    return first + corpus_of(base37(), "b37")


# ── the scan writer ──────────────────────────────────────────────────────────────────────────────────────────────────────────────────
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


class Scan:
    """A gray scan bit by bit, in the Annex K luminance tables (taken from a Pillow file, which carries them)."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.head = DC.pillow_jpeg(H, W, "gray", 75, 0)
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
        at = 1
        for k in sorted(dict(ac)):
            run = k - at
            while run > 15:
                self.zrl()
                run -= 16
            self.ac(run, dict(ac)[k])
            at = k + 1
        return self.eob() if at < 64 else self

    def scan_bytes(self):
        bits = self.bits + [1] * (-len(self.bits) % 8)
        out = bytearray()
        for i in range(0, len(bits), 8):
            b = int("".join(map(str, bits[i:i + 8])), 2)
            out.append(b)
            if b == 0xFF:
                out.append(0)
        return bytes(out)

    def file(self, tail=b""):
        lo, _ = DC.scan_span(self.head)
        return self.head[:lo] + self.scan_bytes() + tail + b"\xff\xd9"


@functools.lru_cache(maxsize=None)
def handmade(H=8, W=64):
    """`{name: (file, claimed status)}` of gray H x W files (at least 8 blocks)."""
    n = Scan(H, W).blocks
    assert n >= 8
    rng = np.random.default_rng(7)

    def filler(s, count):
        for _ in range(count):
            s.block(int(rng.integers(-3, 4)), {int(k): int(rng.integers(-40, 41)) or 1 for k in rng.choice(np.arange(1, 64), 5, replace=False)})
        return s

    cases = {}
    s = Scan(H, W)
    for _ in range(n):
        s.block(1000)
    cases["dc-overflow"] = (s.file(), 4)                          # block 2: 3000 leaves [-2048, 2047]
    s = Scan(H, W)
    for _ in range(5):
        s.block(1000)
    s.raw("1" * 16)
    filler(s, n - 5)
    cases["dc-overflow-then-invalid"] = (s.file(), 4)             # the invalid code three blocks later changes nothing
    s = Scan(H, W)
    s.block(5, {1: 3}).raw("1" * 16)
    for _ in range(n - 1):
        s.block(1000)
    cases["invalid-then-dc-overflow"] = (s.file(), 2)
    s = filler(Scan(H, W), 2)
    s.dc(1).zrl().zrl().zrl().zrl()
    filler(s, n - 3)
    cases["zrl-overflow"] = (s.file(), 3)
    s = filler(Scan(H, W), 1)
    s.dc(1).ac(15, 5).ac(15, 5).ac(15, 5).ac(15, 5)                  # 16, 32, 48, then 64: past the block
    filler(s, n - 2)
    cases["run-overflow"] = (s.file(), 3)
    s = filler(Scan(H, W), n)
    cases["intact"] = (s.file(), 0)
    cases["garbage-before-eoi"] = (s.file(bytes(rng.integers(0, 255, 40, dtype=np.uint8))), 0)      # no 0xFF among them
    body = filler(Scan(H, W), n)
    raw, lo = body.file(), DC.scan_span(body.head)[0]
    mid = lo + (len(raw) - 2 - lo) // 2
    while raw[mid - 1] == 0xFF or raw[mid] == 0xFF:
        mid += 1
    cases["eoi-mid-scan"] = (raw[:mid] + b"\xff\xd9" + raw[mid:], 1)       # the scan ends there: truncated
    cases["app0-mid-scan"] = (raw[:mid] + b"\xff\xe0" + raw[mid:], 6)      # the parser refuses a marker that is not EOI
    cases["rst-mid-scan"] = (raw[:mid] + b"\xff\xd0" + raw[mid:], 5)       # a restart marker in a file without DRI
    return cases
