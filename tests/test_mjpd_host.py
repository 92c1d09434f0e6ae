"""The host twin of the device JPEG decoder (og_jpegd_decode_host, include/decode/openglottal_hip_mjpd.h) against Pillow's libjpeg:
every byte equal over every accepted form; the Annex K rule for files without DHT; every refusal by its reason; and hostile input --
truncations, substitutions, damaged restart markers -- inside guard zones.  No GPU."""
import io
import itertools

import numpy as np
import pytest
from PIL import Image

import buffer_guard as G
import mjpd_cases as DC
from openglottal_amd import mjpeg as MJ
from openglottal_amd._lib import OpenGlottalHipError, lib

SIZES = ((1, 1), (8, 8), (17, 9), (37, 50), (64, 64))


@pytest.mark.parametrize("form", list(DC.FORMS))
@pytest.mark.parametrize("H,W", SIZES)
def test_the_twin_gives_pillows_bytes(H, W, form):
    """Maximum difference 0 over qualities 1..100, restart intervals of 0, 1 and 3 MCUs and per-file Huffman tables."""
    for q, restart, opt in itertools.product((1, 30, 75, 95, 100), (0, 1, 3), (False, True)):
        j = DC.pillow_jpeg(H, W, form, q, restart, opt)
        info = MJ.parse(j)
        assert (info["status"], info["H"], info["W"], info["sampling"], info["Ri"]) == (0, H, W, DC.SAMPLING[form], restart), (q, restart, opt)
        got, st = MJ.decode_host(j, statuses=True)
        assert st == 0 and np.array_equal(got, DC.pillow_bgr(j)), (H, W, form, q, restart, opt)


def test_narrow_components_are_replicated_as_libjpeg_does():
    """libjpeg upsamples a chroma plane of one or two columns by plain replication; three columns are the first fancy case."""
    for (H, W), form in itertools.product(((2, 3), (3, 4), (5, 5), (4, 6), (3, 2), (16, 1)), ("422", "420")):
        j = DC.pillow_jpeg(H, W, form, 90)
        assert np.array_equal(MJ.decode_host(j), DC.pillow_bgr(j)), (H, W, form)


@pytest.mark.parametrize("H,W", ((13, 21), (40, 56), (64, 64)))
def test_the_files_of_our_own_encoder(H, W):
    j = MJ.encode_host(DC.noise(H, W), 75)
    info = MJ.parse(j)
    assert (info["Ri"], info["sampling"], info["nI"]) == (16, 1, -(-info["M"] // 16))
    assert np.array_equal(MJ.decode_host(j), DC.pillow_bgr(j))


def test_a_file_without_dht_is_decoded_with_the_annex_k_tables():
    for form in DC.FORMS:
        j = DC.pillow_jpeg(17, 9, form, 75, 1, False)
        bare = DC.strip_dht(j)
        assert len(bare) < len(j) and MJ.parse(j)["tables"] & 0x330 and not MJ.parse(bare)["tables"] & 0x330
        assert np.array_equal(MJ.decode_host(bare), MJ.decode_host(j))
        # IJG libjpeg refuses such a file ("Huffman table was not defined"): why the rule exists.  libjpeg-turbo installs the same
        # Annex K tables itself; a Pillow built on it must then give the same pixels.  One of the two holds.
        try:
            ref = DC.pillow_bgr(bare)
        except Exception as e:
            assert "uffman" in str(e) or "broken" in str(e)
        else:
            assert np.array_equal(ref, MJ.decode_host(bare)), form


def _patched(j, marker, rel, value):
    at = j.index(marker) + rel
    return j[:at] + bytes([value]) + j[at + 1:]


def _refusals():
    base = DC.pillow_jpeg(16, 16, "444")
    b = io.BytesIO()
    Image.fromarray(DC.noise(16, 16)).save(b, "JPEG", progressive=True)
    sof, dqt, sos = b"\xff\xc0", b"\xff\xdb", b"\xff\xda"
    cmyk = io.BytesIO()
    Image.fromarray(np.zeros((8, 8, 4), np.uint8), "CMYK").save(cmyk, "JPEG")
    return {
        "progressive": (b.getvalue(), "progressive"),
        "SOF1": (_patched(base, sof, 1, 0xC1), "SOF1"),
        "SOF3": (_patched(base, sof, 1, 0xC3), "SOF3"),
        "SOF9 (arithmetic)": (_patched(base, sof, 1, 0xC9), "SOF9"),
        "12 bit": (_patched(base, sof, 4, 12), "12-bit"),
        "4:4:0": (_patched(base, sof, 11, 0x12), "sampling factors 1x2"),
        "4:1:1": (_patched(base, sof, 11, 0x41), "sampling factors 4x1"),
        "chroma 2x1": (_patched(base, sof, 14, 0x21), "sampling factors"),
        "four components": (cmyk.getvalue(), "4 components"),
        "16-bit DQT": (_patched(base, dqt, 4, 0x10), "16-bit quantisation"),
        "H of 0": (_patched(_patched(base, sof, 5, 0), sof, 6, 0), "H or W of 0"),
        "W of 0": (_patched(_patched(base, sof, 7, 0), sof, 8, 0), "H or W of 0"),
        "H * W above the limit": (_patched(_patched(base, sof, 5, 0x20), sof, 7, 0x20), "above"),
        "spectral selection": (_patched(base, sos, 11, 1), "spectral selection"),
        "a scan of one component": (base[:base.index(sos) + 4] + b"\x01" + base[base.index(sos) + 5:], "several scans"),
        "a second scan": (base[:-2] + base[base.index(sos):], "several scans"),
        "no SOI": (b"\x00" + base[1:], "no SOI"),
        "no SOS": (base[:base.index(sos)], "no SOS"),
        "a table that is not defined": (_patched(base, sof, 12, 3), "not defined"),
    }


@pytest.mark.parametrize("name", list(_refusals()))
def test_every_refusal_by_its_reason(name):
    j, why = _refusals()[name]
    info = MJ.parse(j)
    assert info["status"] == 6 and why in info["why"], (name, info)
    assert MJ.decode_host(j, statuses=True) == (None, 6)
    with pytest.raises(OpenGlottalHipError, match="refuses"):
        MJ.decode_host(j)
    # the twin itself: status 6, nothing written
    rc, pay, faults = G.guarded_call(lambda p: lib().og_jpegd_decode_host(p["j"], len(j), p["out"], 1 << 16, p["st"]),
                                     {"j": np.frombuffer(j, np.uint8)}, {"out": 1 << 16, "st": 4})
    assert rc == 0 and not faults and pay["st"].view(np.int32)[0] == 6 and (pay["out"] == G.GUARD_FILL).all()


def test_the_base_of_the_refusals_is_accepted():
    j = DC.pillow_jpeg(16, 16, "444")
    assert MJ.parse(j)["status"] == 0 and MJ.parse(_patched(j, b"\xff\xc0", 1, 0xC0))["status"] == 0


def test_hostile_input_terminates_inside_its_buffers_with_a_listed_status():
    """Every truncation, 500 substitutions in the scan per file, a removed, a doubled and a renumbered RSTm: the input and the output
    lie between guard zones; every canary stays, and the result is status 0 with a whole frame, a listed status, or a refusal (6)
    that writes nothing."""
    H, W = 17, 9
    seen = set()
    for label, j in DC.hostile():
        src = np.frombuffer(j, np.uint8) if j else np.zeros(0, np.uint8)
        inp = G.Region("jpeg", max(len(j), 1), "host", G.GUARD_MIN, 0xFF)       # (0xFF slack: a read past the end would meet a marker prefix)
        inp._raw[inp.lo:inp.lo + len(j)] = src
        out = G.Region("out", H * W * 3, "host", G.GUARD_MIN, G.GUARD_FILL)
        st = G.Region("st", 4, "host", G.GUARD_MIN, G.GUARD_FILL)
        before = inp.snapshot()
        rc = lib().og_jpegd_decode_host(inp.ptr, len(j), out.ptr, H * W * 3, st.ptr)
        assert rc == 0, label
        assert np.array_equal(inp.snapshot(), before), label
        for r in (out, st):
            assert not r.dirty(0, r.lo).size and not r.dirty(r.hi, len(r._raw)).size, (label, r.name)
        status = int(st.payload().view(np.int32)[0])
        seen.add(status)
        if status == 6:
            assert (out.payload() == G.GUARD_FILL).all(), label
        else:
            assert status == 0 or status in DC.LISTED, (label, status)
            assert np.array_equal(out.payload().reshape(H, W, 3), DC.twin(j)[0]), label      # a whole frame, and the same one every time
    assert {0, 1, 2, 3, 5, 6} <= seen
    for label in ("ri1-rst-removed", "ri1-rst-doubled", "ri1-rst-renumbered"):
        assert DC.twin(dict(DC.hostile())[label])[1] == 5


def test_what_pillow_does_far_outside_the_sample_range():
    """libjpeg's C code limits samples through a table that wraps modulo 1024; the answer that counts is Pillow's.  Samples of
    128 + dc * q / 8: up to four times the range past either end Pillow saturates, as the twin's clamp does (the C table would give 0
    at 638 + 128).  Parity stops where Pillow's 16-bit first pass overflows (|4 * dc * q| >= 2^15); the header says so."""
    for dc, q in ((5, 255), (12, 255), (16, 255), (20, 255), (28, 255), (-5, 255), (-16, 255), (-20, 255), (-21, 255), (300, 16), (-300, 16)):
        j = DC._handmade_gray(dc, q)
        assert abs(4 * dc * q) < 1 << 15
        want = DC.pillow_bgr(j)
        assert np.array_equal(MJ.decode_host(j), want), (dc, q)
        assert (want == (255 if dc > 0 else 0)).all()
    # far outside: the twin still answers, with status 0 and a clamped frame; no parity is claimed there
    for dc in (1023, -1023, 2047, -2047):
        f, st = MJ.decode_host(DC._handmade_gray(dc, 255), statuses=True)
        assert st == 0 and f.shape == (8, 8, 3)


def test_the_int32_bound_of_the_header():
    """The header's BOUND paragraph: every intermediate of og_jpegd_idct8 as a linear form of the 8 inputs, the largest Euclidean norm
    of a weight vector, and the E it allows.  The walk below is held to the code: the eight results it ends with must be the weights
    that og_jpegd_idct_pass_host (the function the twin and k_mjpd_idct run) has, read off unit inputs; and the pass is linear there."""
    norms = []

    def rec(v):
        norms.append(float(np.linalg.norm(v)))
        return v

    x = list(np.eye(8))
    z1 = rec(rec(x[2] + x[6]) * 4433)
    tmp2, tmp3 = rec(z1 + rec(x[6] * -15137)), rec(z1 + rec(x[2] * 6270))
    tmp0, tmp1 = rec(rec(x[0] + x[4]) * 8192), rec(rec(x[0] - x[4]) * 8192)
    tmp10, tmp13, tmp11, tmp12 = rec(tmp0 + tmp3), rec(tmp0 - tmp3), rec(tmp1 + tmp2), rec(tmp1 - tmp2)
    t0, t1, t2, t3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = rec(t0 + t3), rec(t1 + t2), rec(t0 + t2), rec(t1 + t3)
    z5 = rec(rec(z3 + z4) * 9633)
    t0, t1, t2, t3 = rec(t0 * 2446), rec(t1 * 16819), rec(t2 * 25172), rec(t3 * 12299)
    z1, z2, z3, z4 = rec(z1 * -7373), rec(z2 * -20995), rec(z3 * -16069 + 0), rec(z4 * -3196)
    z3, z4 = rec(z3 + z5), rec(z4 + z5)
    t0, t1, t2, t3 = rec(rec(z1 + z3) + t0), rec(rec(z2 + z4) + t1), rec(rec(z2 + z3) + t2), rec(rec(z1 + z4) + t3)
    outs = [rec(v) for v in (tmp10 + t3, tmp10 - t3, tmp11 + t2, tmp11 - t2, tmp12 + t1, tmp12 - t1, tmp13 + t0, tmp13 - t0)]
    assert all(abs(np.linalg.norm(o) - 8192 * 8 ** 0.5) < 1 for o in outs)      # 2^13 sqrt(8) times an orthonormal transform

    def run(v, shift):
        a, o = np.asarray(v, np.int32), np.zeros(8, np.int32)
        assert lib().og_jpegd_idct_pass_host(a.ctypes.data, shift, o.ctypes.data) == 0
        return o

    # an input of 2^11 e_k through the column pass: (2^11 w + 2^10) >> 11 = w, exactly
    code = np.stack([run(2048 * np.eye(8, dtype=np.int32)[k], 11) for k in range(8)], axis=1)      # [result][input]
    walk = np.stack([outs[i] for i in (0, 2, 4, 6, 7, 5, 3, 1)])                                   # results 0..7 in the code's order
    assert np.array_equal(code, walk.astype(np.int64))
    rs = np.random.RandomState(3)
    for shift in (11, 18):                                                 # and the pass IS that linear form, rounded, on any input in range
        for _ in range(50):
            v = rs.randint(-2000, 2001, 8)
            assert np.array_equal(run(v, shift), (walk.astype(np.int64) @ v + (1 << (shift - 1))) >> shift)
    assert lib().og_jpegd_idct_pass_host(None, 11, code.ctypes.data) == -1 and lib().og_jpegd_idct_pass_host(code.ctypes.data, 12, code.ctypes.data) == -1
    W = max(norms)
    assert 31871 < W < 31872
    E = 5900
    assert 31872 * E + 2 ** 10 < 2 ** 31 and 31872 * (11.32 * E + 4) + 2 ** 17 < 2 ** 31 and 4 * 8 ** 0.5 < 11.32
    assert 1024 + 255 * 8 / 2 < E                                            # any file encoded from pixels, any 8-bit table


# ── the files of tests/test_gpu_mjpd.py's marker, lane-map, plane and code cases: what each is named for, on the CPU ───────────────────
def _twin_is_pillows(j, label):
    f, st = DC.twin(j)
    assert st == 0 and np.array_equal(f, DC.pillow_bgr(j)), label


def test_marker_placements_hold_on_the_bytes_and_the_files_are_pillows():
    """Every valid restart-scan file: the builder asserts its placement (strides, wave slices, residues of the marker's FF and of the
    scan's length mod 256) on the bytes it returns; the twin gives status 0 and Pillow's bytes."""
    files = DC.valid_placements()
    assert len(files) == 4 + 2 * len(DC.EDGES) + len(DC.LENGTHS) and len({j for _, j in files}) == len(files)
    for label, j in files:
        _twin_is_pillows(j, label)
    assert not np.array_equal(DC.twin(DC.dense(0))[0], DC.twin(DC.dense(1))[0])
    assert {R for R in DC.EDGES} == {(255,), (254,), (0,), (63, 64), (0, 255)} and set(DC.LENGTHS) == {0, 1, 255}
    for seed in (0, 1):
        assert DC.empty_strides(DC.sparse(seed)) and not DC.empty_strides(DC.dense(seed)) and not DC.empty_slices(DC.dense(seed))


def test_damaged_markers_have_their_claimed_status_and_a_whole_frame():
    """The seven damages of dense(0): the twin's status is the claimed one (5, and 0 for the scan that ends in a lone FF), and the frame
    is written whole between its guard zones -- mid-gray for 5, since no interval is decoded."""
    H, W = 8, 2400
    cases = DC.damaged()
    assert set(cases) == {"renumbered-late", "renumbered-by-4", "mod7", "removed-last", "doubled-all", "end-marker", "ff-last"}
    for name, (j, claim) in cases.items():
        assert MJ.parse(j)["status"] == 0 and DC.twin(j)[1] == claim == (0 if name == "ff-last" else 5), name
        out = G.run_guarded("og_jpegd_decode_host", name, lambda p: lib().og_jpegd_decode_host(p["j"], len(j), p["out"], H * W * 3, p["st"]),
                            {"j": np.frombuffer(j, np.uint8)}, {"out": H * W * 3, "st": 4})
        assert out["st"].view(np.int32)[0] == claim
        frame = out["out"].reshape(H, W, 3)
        assert np.array_equal(frame, DC.twin(j)[0])
        if claim == 5:
            assert (frame == 128).all(), name
        else:
            assert np.array_equal(frame, DC.twin(DC.dense(0))[0])       # the missing EOI takes nothing from the last interval
    assert [DC.twin(j)[1] for j in DC.guard_batch()] == DC.GUARD_STATUS


def test_the_lane_map_files():
    files = DC.lane_files()
    for j in files:
        _twin_is_pillows(j, "lane")
    assert DC.twin(DC.rst_removed(files[5]))[1] == 5 and MJ.parse(DC.rst_removed(files[5]))["nI"] == 12
    for nI, lane64 in ((3, (21, 1)), (20, (3, 4))):
        batch, at = DC.lane_batch(nI)
        assert at == lane64 and at[1] != 0                   # the second workgroup's first lane is not a frame's first interval
        for j in set(batch):
            _twin_is_pillows(j, nI)


def test_narrow_planes_at_three_seeds():
    assert {(W + 1) // 2 for _, W, form in DC.NARROW if form in ("422", "420")} == {1, 2, 3}     # both sides of cw <= 2
    for H, W, form in DC.NARROW:
        for j in DC.narrow_files(H, W, form):
            assert (MJ.parse(j)["H"], MJ.parse(j)["W"], MJ.parse(j)["sampling"]) == (H, W, DC.SAMPLING[form])
            _twin_is_pillows(j, (H, W, form))


def test_long_codes_are_in_the_files_that_claim_them():
    """The lengths come from the file's own DHT: with the Annex K luminance AC table 9, 10, 11, 12, 15 and 16 bits.  A code of 10 bits
    or more misses the 9-bit look-up and is found by the maxcode walk."""
    j, lengths = DC.long_codes()
    assert lengths == tuple(DC.long_lengths(DC._dht(j)[(1, 0)])) and set(lengths) >= {9, 10, 16} and len(lengths) == 6
    _twin_is_pillows(j, "long codes")
    assert len(np.unique(DC.twin(j)[0])) > 8
    _twin_is_pillows(DC.long_chroma(), "optimised chroma tables")


def test_past_the_bound_the_twin_still_answers():
    """Every quantisation step 255, DC at both ends of its range, every AC value +-1023: far outside the header's BOUND, where only
    device = twin is claimed (Pillow differs in about half the bytes)."""
    j = DC.past_the_bound()
    assert MJ.parse(j)["status"] == 0 and (MJ.parse(j)["H"], MJ.parse(j)["W"]) == (8, 64)
    f, st = DC.twin(j)
    assert st == 0 and f.shape == (8, 64, 3) and len(np.unique(f)) > 1
