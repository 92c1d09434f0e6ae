"""Inputs of the split entropy decoder's tests (helper module beside tests/mjpd_cases.py, whose Pillow files and hostile corpus it
reuses): the (sub, lanes) pairs of the issue, a second hostile corpus from a 37x50 4:2:0 file without DRI, and hand-made gray files
from mjpd_cases' Annex-K scan writer -- coefficient blocks and raw bits in, bytes out -- whose claimed statuses the sequential twin
confirms; and the files of the kernel's windows -- Pillow noise of two and three real 32 768-byte windows, hand-made scans whose bytes
a seeded search places on window edges, errors behind window 0 -- each with the firing check that the tests assert.  Everything is
cached."""
import functools
import time

import numpy as np

import mjpd_cases as DC
from mjpd_cases import Scan, _dht, pack_bits      # noqa: F401  (the writer lives beside the Pillow files; the restart-scan writer there builds on it)
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


# ── hand-made scans (the writer is mjpd_cases.Scan) ──────────────────────────────────────────────────────────────────────────────────
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


# ── the kernel's windows ─────────────────────────────────────────────────────────────────────────────────────────────────────────────
# k_mjps_entropy walks a scan in windows of lanes_of(sub) subsequences and stages SLACK bytes behind each.  What follows builds files
# whose bytes lie where the windows' edges are decided, and states each placement as a predicate that the tests assert.
WINDOW, SLACK = 32768, 16                       # og_mjps_limit(4); the bytes staged behind a window
SUBS = (64, None, 256, 512, 1024)               # None: the default, 128
EXTRA = ((256, 256), (512, 256), (128, 256))    # beside PAIRS in the CPU half
ENDS = ("Wn-1", "Wn", "Wn+1", "Wn+K-1", "Wn+K", "Wn+K+1")
AFTER_END = b"\xff\xff\x00" + bytes(range(1, 41))   # a fill FF before a stuffed pair: the parser walks on, the data ends at the first FF
BUILD_SECONDS = {}


def lanes_of(sub):
    """The kernel's lanes per window."""
    return min(256, WINDOW // (sub or MJ.split_limit(0)))


def window_of(sub):
    return lanes_of(sub) * (sub or MJ.split_limit(0))


def scan_of(jpeg):
    lo, hi = DC.scan_span(jpeg)
    return bytes(jpeg[lo:hi])


def data_end(scan):
    """Index of the first 0xFF that is no stuffed pair (the scan's length if there is none): where og_jpegd_fill stops."""
    i = scan.find(b"\xff")
    while i >= 0 and i + 1 < len(scan) and scan[i + 1] == 0:
        i = scan.find(b"\xff", i + 2)
    return len(scan) if i < 0 else i


@functools.lru_cache(maxsize=None)
def kernel_twin(jpeg, sub):
    """`(frame, status, stats)` of the split twin at the kernel's own lanes per window."""
    out, st, stats = split(jpeg, sub or 0, lanes_of(sub), stats=True)
    if out is not None:
        out.setflags(write=False)
    return out, st, stats


def pairs_for(jpeg):
    """PAIRS and EXTRA; a file above 32 KB keeps 256 lanes, so that the twin's window is the kernel's."""
    pairs = PAIRS + EXTRA
    if MJ.parse(jpeg)["scan_length"] > WINDOW:
        pairs = tuple(dict.fromkeys((sub, 256) for sub, _ in pairs))
    return pairs


def dense(rng, nac, amp=40):
    """`{zigzag index: value}` of `nac` non-zero AC values up to `amp` in magnitude."""
    ks = rng.choice(np.arange(1, 64), nac, replace=False)
    return {int(k): int(rng.integers(1, amp + 1)) * (1 if rng.integers(2) else -1) for k in ks}


def fill(s, rng, count, nac=40, amp=40):
    for _ in range(count):
        s.block(int(rng.integers(-3, 4)), dense(rng, nac, amp))
    return s


def search(H, W, pred, nacs=(40,), seeds=range(48), near=None, tail=b"", accept=None, blocks=None, whole=False):
    """The gray H x W file (its scan followed by `tail`) of the first (AC values per block, seed, first block) whose written scan
    satisfies `pred(scan bytes)` -- and whose file satisfies `accept(file)`, if that is given.  The blocks behind the first are
    dense filler from `seed`; the first block takes 0..63 AC values of ten magnitudes, and every bit length of it shifts all the
    bytes behind it.  `near`: a wanted scan length, to skip fillers that cannot reach it.  `blocks`: how many blocks are
    written (all of the frame's unless given); `whole`: only scans whose bits fill their last byte, so that no padding follows the
    last symbol.  Seeded and deterministic; raises if nothing fires."""
    s = Scan(H, W)
    lo = DC.scan_span(s.head)[0]
    for nac in nacs:
        for seed in seeds:
            s.bits = []
            fill(s, np.random.default_rng([H, W, nac, seed]), (blocks or s.blocks) - 1, nac)
            body = np.asarray(s.bits, np.uint8)
            if near is not None and not near - near // 8 - 260 <= body.size // 8 <= near:      # (stuffing adds a few per cent)
                continue
            seen = set()
            for n0 in range(64):
                for amp in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512):
                    rng = np.random.default_rng([seed, n0, amp])
                    s.bits = []
                    s.block(int(rng.integers(-3, 4)), dense(rng, n0, amp))
                    if (whole and (len(s.bits) + body.size) % 8) or len(s.bits) in seen or (near is not None and not near - near // 8 <= (len(s.bits) + body.size + 7) // 8 <= near):
                        continue
                    seen.add(len(s.bits))
                    scan = pack_bits(np.concatenate([np.asarray(s.bits, np.uint8), body]))
                    if pred(scan) and (accept is None or accept(s.head[:lo] + scan + tail + b"\xff\xd9")):
                        return s.head[:lo] + scan + tail + b"\xff\xd9"
    raise AssertionError(f"no {H} x {W} scan satisfies the predicate")


def stuffed_at(scan, i):
    """A stuffed pair whose FF is byte i."""
    return 0 < i + 1 < len(scan) and scan[i] == 0xFF and scan[i + 1] == 0


# section 3 of the issue, a to c and e: name -> predicate(scan, sub).  Every file has at least three windows.
EDGES = {
    "pair-across-Wn": lambda scan, sub: stuffed_at(scan, window_of(sub) - 1),
    "pair-across-2Wn": lambda scan, sub: stuffed_at(scan, 2 * window_of(sub) - 1),
    "pair-ends-the-slack": lambda scan, sub: stuffed_at(scan, window_of(sub) + SLACK - 1),
    "pair-on-a-dword-edge-in-window-1": lambda scan, sub: any(stuffed_at(scan, i) for i in range(window_of(sub) + 3, 2 * window_of(sub), 4)),
    "lane-starts-on-the-00-in-window-1": lambda scan, sub: any(stuffed_at(scan, window_of(sub) + sub * k - 1) for k in range(1, lanes_of(sub))),
}
EDGE_SHAPE = {4: (64, 64), 8: (64, 128)}     # 64 and 128 dense blocks of some 60 bytes: four windows or more
END_SHAPE = {4: (24, 48), 8: (40, 56)}      # 18 and 35 blocks of 30 AC values or more: a complete frame of about one window


@functools.lru_cache(maxsize=None)
def edge_case(name, sub):
    H, W = EDGE_SHAPE[sub]
    return search(H, W, lambda scan: len(scan) > 2 * window_of(sub) + SLACK and EDGES[name](scan, sub))


def end_offset(name, sub):
    Wn, K = window_of(sub), SLACK
    return {"Wn-1": Wn - 1, "Wn": Wn, "Wn+1": Wn + 1, "Wn+K-1": Wn + K - 1, "Wn+K": Wn + K, "Wn+K+1": Wn + K + 1}[name]


@functools.lru_cache(maxsize=None)
def end_case(name, sub):
    """A COMPLETE frame (status 0) whose data is exactly end_offset bytes: the first FF that is no stuffed pair follows them, and 42
    bytes that no decoder reads lie behind it, so that the kernel's search has to find that FF.  With the end behind Wn the frame's
    last symbol starts at or behind Wn: the decoder needs the second window, of 1 to 17 bytes (windows == 2 in the twin's stats)."""
    H, W = END_SHAPE[sub]
    e = end_offset(name, sub)
    return search(H, W, lambda scan: len(scan) == e, nacs=range(30, 63), seeds=range(4), near=e, tail=AFTER_END,
                  accept=lambda j: split(j, sub, lanes_of(sub), stats=True)[2]["windows"] == (2 if e > window_of(sub) else 1))


@functools.lru_cache(maxsize=None)
def three_windows_at_1024(H=128, W=192):
    """A hand-made gray scan of three windows at sub 1024: 384 blocks of 63 AC values of ten bits.  BUILD_SECONDS: what the writer took."""
    t0 = time.perf_counter()
    s = Scan(H, W)
    fill(s, np.random.default_rng([H, W]), s.blocks, 63, 1023)
    j = s.file()
    BUILD_SECONDS["three-windows-at-1024"] = time.perf_counter() - t0
    return j


def _at(s):
    """Bytes of the scan that the bits written so far fill."""
    return len(pack_bits(s.bits[:len(s.bits) // 8 * 8]))


def _fill_to(s, rng, target, nac=40):
    """Dense blocks until the scan has reached `target` bytes; returns the blocks written."""
    count = 0
    while len(s.bits) // 8 < target - 8 or _at(s) < target:
        fill(s, rng, 1, nac)
        count += 1
    return count


@functools.lru_cache(maxsize=None)
def late_errors(sub, H=64, W=128):
    """`{name: (file, status, offset)}`: gray H x W files whose first error lies behind window 0 at `sub`; `offset` is the byte of the
    scan where the injected bits (or the cut) begin.  The running DC predictor stays inside [-2048, 2047] before the overflow."""
    Wn, n = window_of(sub), Scan(H, W).blocks
    cases = {}
    s = fill(Scan(H, W), np.random.default_rng([sub, 0]), n)
    intact = s.file()
    assert len(s.scan_bytes()) > 3 * Wn
    cases["intact"] = (intact, 0, None)
    cut = Wn + Wn // 2
    cases["truncated-in-window-1"] = (intact[:DC.scan_span(intact)[0] + cut], 1, cut)
    rng = np.random.default_rng([sub, 1])
    s = Scan(H, W)
    k = _fill_to(s, rng, 2 * Wn + Wn // 4)
    at = _at(s)
    fill(s.raw("1" * 16), rng, n - k)
    cases["invalid-code-in-window-2"] = (s.file(), 2, at)
    rng = np.random.default_rng([sub, 2])
    s = Scan(H, W)
    k = _fill_to(s, rng, Wn + Wn // 4)
    assert k >= 4 and 3 * k < 1000                     # |predictor| <= 3 per block before: far from the range's ends
    for _ in range(2):
        s.block(1000, dense(rng, 40))
    at = _at(s)                                        # the third: 3000 + (at most 3 k) leaves the range
    s.block(1000, dense(rng, 40))
    fill(s, rng, n - k - 3)
    cases["dc-overflow-in-window-1"] = (s.file(), 4, at)
    rng = np.random.default_rng([sub, 3])
    s = Scan(H, W)
    k = _fill_to(s, rng, Wn + Wn // 2)
    at = _at(s)
    s.dc(1).zrl().zrl().zrl().zrl()
    fill(s, rng, n - k - 1)
    cases["zrl-overflow-in-window-1"] = (s.file(), 3, at)
    return cases


LATE = {"truncated-in-window-1": 1, "invalid-code-in-window-2": 2, "dc-overflow-in-window-1": 1, "zrl-overflow-in-window-1": 1}   # name -> window
LATE_BATCHES = (("intact", "truncated-in-window-1", "invalid-code-in-window-2", "intact"),
                ("intact", "dc-overflow-in-window-1", "zrl-overflow-in-window-1", "intact"))


@functools.lru_cache(maxsize=None)
def cut_case(name, sub):
    """late_errors' intact file cut (no EOI) so that its scan is end_offset bytes: a TRUNCATED frame whose bytes end at the window's
    edge without any FF to find.  At "Wn" the scan is exactly one window and only its open last lane can report the missing bits."""
    intact = late_errors(sub)["intact"][0]
    return intact[:DC.scan_span(intact)[0] + end_offset(name, sub)]


SYMBOL_EDGE_SHAPE = {4: ((32, 48), 18), 8: ((48, 56), 35)}      # (frame, blocks written): 24 and 42 blocks, 6 and 7 of them missing


@functools.lru_cache(maxsize=None)
def symbol_edge_case(sub):
    """A truncated frame whose scan is exactly Wn bytes AND ends on a symbol's last bit (`whole`: no padding bit behind it, no FF to
    find): the reader is empty at the window's end, so only a last lane whose end is open asks for the next symbol and meets the
    missing bits.  With `last` false at n == Wn the kernel would leave its window loop with status 0."""
    (H, W), blocks = SYMBOL_EDGE_SHAPE[sub]
    Wn = window_of(sub)
    return search(H, W, lambda scan: len(scan) == Wn, nacs=range(30, 63), seeds=range(4), near=Wn, blocks=blocks, whole=True)


def symbol_edge_fires(sub):
    j = symbol_edge_case(sub)
    (H, W), blocks = SYMBOL_EDGE_SHAPE[sub]
    scan = scan_of(j)
    assert blocks < Scan(H, W).blocks and len(scan) == data_end(scan) == window_of(sub)
    _, st, stats = kernel_twin(j, sub)
    assert DC.twin(j)[1] == st == 1 and stats["windows"] == 1 and stats["lanes"] == lanes_of(sub)
    return j      # (that no padding bit follows the last symbol is `whole`'s doing in search(): the bytes alone do not tell)


MIXED_CUT = WINDOW + WINDOW // 4     # inside the second window at sub 256 (and the forty-first at sub 4)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """128 x 128 4:4:4 noise without DRI, the quality alone differing: two files of three windows at sub 256, one of a single short
    window (quality 1), one more of three windows, and the first one cut inside its second window."""
    long = [DC.pillow_jpeg(128, 128, "444", 100, 0, False, s) for s in range(3)]
    short = DC.pillow_jpeg(128, 128, "444", 1, 0, False, 3)
    cut = long[0][:DC.scan_span(long[0])[0] + MIXED_CUT]
    return (long[0], long[1], short, long[2], cut)


# the Pillow files of real windows: name -> (H, W, form, the subs they run at, windows at least -- at every one of those subs)
REAL = {"444-128x128": (128, 128, "444", SUBS, 2), "444-128x192": (128, 192, "444", SUBS, 3),
        "420-128x192": (128, 192, "420", (1024, 256), 2), "gray-128x192": (128, 192, "gray", (1024, 256), 2)}


def real(name):
    H, W, form, _, _ = REAL[name]
    return DC.pillow_jpeg(H, W, form, 100, 0)


# ── the firing checks: a case that no longer holds what it is named for fails here, in the CPU suite and again beside the GPU run ────
def real_fires(name):
    H, W, form, subs, least = REAL[name]
    j = real(name)
    info = MJ.parse(j)
    assert (info["H"], info["W"], info["Ri"], info["sampling"]) == (H, W, 0, DC.SAMPLING[form])
    if name == "444-128x128":
        assert info["scan_length"] > WINDOW
    if name == "444-128x192":
        assert info["scan_length"] >= 2 * WINDOW + 1          # (128 x 192 suffices: nothing had to grow)
    for sub in subs:
        _, st, stats = kernel_twin(j, sub)
        assert st == 0 and stats["windows"] >= least, (name, sub, stats)
        assert stats["windows"] == -(-stats["lanes"] // lanes_of(sub))
        if (sub or 0) >= 256:                                   # lanes, at 1024 whole waves, idle inside a full window
            assert lanes_of(sub) == WINDOW // sub < 256 and stats["lanes"] > lanes_of(sub)
    return j


def edge_fires(name, sub):
    j = edge_case(name, sub)
    scan = scan_of(j)
    assert EDGES[name](scan, sub), (name, sub)
    assert data_end(scan) == len(scan) > 2 * window_of(sub) + SLACK
    _, st, stats = kernel_twin(j, sub)
    assert DC.twin(j)[1] == st == 0 and stats["windows"] >= 3
    return j


def end_fires(name, sub):
    j = end_case(name, sub)
    scan, e, Wn = scan_of(j), end_offset(name, sub), window_of(sub)
    assert data_end(scan) == e and scan[e:e + 2] == b"\xff\xff" and len(scan) == e + len(AFTER_END)
    _, st, stats = kernel_twin(j, sub)
    assert DC.twin(j)[1] == st == 0                            # a complete frame at every one of the six offsets
    # at or before Wn window 0 is the last; behind it a second window of 1 .. 17 bytes follows, one lane at sub 4 .. K
    assert stats["windows"] == (1 if e <= Wn else 2)
    assert stats["lanes"] == (-(-e // sub) if e <= Wn else lanes_of(sub) + -(-(e - Wn) // sub))
    return j


def cut_fires(name, sub):
    j = cut_case(name, sub)
    e = end_offset(name, sub)
    assert MJ.parse(j)["scan_length"] == e and DC.twin(j)[1] == 1
    _, st, stats = kernel_twin(j, sub)
    # (behind Wn the missing bits are met in window 0 already if the symbol that lacks them starts there)
    assert st == 1 and stats["windows"] in ((1,) if e <= window_of(sub) else (1, 2))
    return j


def late_fires(name, sub):
    j, claim, at = late_errors(sub)[name]
    _, st, stats = kernel_twin(j, sub)
    assert DC.twin(j)[1] == st == claim, (name, sub)
    if name == "intact":
        assert stats["windows"] >= 3
    else:
        k, Wn = LATE[name], window_of(sub)
        assert k * Wn + SLACK <= at < (k + 1) * Wn - SLACK, (name, sub, at)      # well inside window k: no slack of window k - 1 holds it
        assert stats["windows"] == k + 1                                          # the windows behind the error are not decoded
        assert (MJ.parse(j)["scan_length"] == at) == (name == "truncated-in-window-1")
    return j


def mixed_fires(sub):
    files = mixed_batch()
    assert all((i["H"], i["W"], i["sampling"], i["Ri"]) == (128, 128, 1, 0) for i in map(MJ.parse, files))
    assert [DC.twin(j)[1] for j in files] == [kernel_twin(j, sub)[1] for j in files] == [0, 0, 0, 0, 1]
    windows = [kernel_twin(j, sub)[2]["windows"] for j in files]
    if sub == 256:
        assert windows == [3, 3, 1, 3, 2] and MJ.parse(files[2])["scan_length"] < 2048
    else:
        assert sub == 4 and windows[2] == 2 and all(w >= 40 for i, w in enumerate(windows) if i != 2)
    assert MJ.parse(files[4])["scan_length"] == MIXED_CUT and MIXED_CUT // window_of(sub) >= 1
    return files


GROUPS = ("real", "mixed", "edges-4", "edges-8", "ends-4", "ends-8", "cuts-4", "cuts-8", "late-4", "late-8", "three-windows-at-1024")


def group(name):
    """`[(label, file)]`: every file the window tests build, by group (each built once per process)."""
    kind, _, sub = name.partition("-")
    sub = int(sub) if sub.isdigit() else None
    if kind == "real":
        return [(n, real(n)) for n in REAL]
    if kind == "mixed":
        return [(f"mixed{i}", j) for i, j in enumerate(mixed_batch())]
    if kind == "edges":
        return [(n, edge_case(n, sub)) for n in EDGES]
    if kind == "ends":
        return [(n, end_case(n, sub)) for n in ENDS]
    if kind == "cuts":
        return [(n, cut_case(n, sub)) for n in ENDS] + [("on-a-symbol-edge", symbol_edge_case(sub))]
    if kind == "late":
        return [(n, j) for n, (j, _, _) in late_errors(sub).items()]
    return [(name, three_windows_at_1024())]
