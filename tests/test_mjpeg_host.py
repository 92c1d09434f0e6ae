"""The host twin of include/openglottal_hip_mjpeg.h against two references it shares no code with: Pillow (libjpeg's tables, decoder
and encoder) and the models of tests/mjpeg_cases.py (a strict scan decoder, a float64 transform).  No GPU.  The device is held to the
twin byte for byte in tests/test_gpu_mjpeg.py."""
import collections
import io

import numpy as np
import pytest
from PIL import Image

import mjpeg_cases as MC
from openglottal_amd import mjpeg as MJ

QUALITIES = (1, 10, 25, 50, 75, 90, 95, 100)
# The largest shortfall of the twin's PSNR against libjpeg's own encoding at the same tables, measured over the matrix and rounded up
# to the next 0.05 dB (DESIGN.md section 22 has the per-case values).  Both are exact-to-rounding forms of one transform.
PSNR_MARGIN_DB = 0.10                                                     # measured: 0.084 dB (ri+1-ramp, 876 bytes of file)


def test_quantisation_tables_are_the_ones_pillow_writes():
    for q in QUALITIES:
        ql, qc, _ = MJ.tables(q)
        b = io.BytesIO()
        Image.new("RGB", (16, 16)).save(b, "JPEG", quality=q, subsampling=0)
        theirs = Image.open(io.BytesIO(b.getvalue())).quantization
        assert list(ql) == list(theirs[0]) and list(qc) == list(theirs[1]), q
        # and the header carries them: DQT is parsed back to natural order by the reader
        h = MC.parse(MJ.encode_host(np.zeros((8, 8, 3), np.uint8), q))
        assert h["q"] == {0: list(ql), 1: list(qc)}, q


def test_huffman_tables_are_the_ones_of_a_pillow_file():
    b = io.BytesIO()
    Image.new("RGB", (16, 16)).save(b, "JPEG", quality=75, subsampling=0, optimize=False)
    theirs = MC.parse(b.getvalue())
    ql, qc, hdr = MJ.tables(75, 16, 16)
    ours = MC.parse(hdr)
    assert len(ours["dht"]) == 4 and ours["dht"] == theirs["dht"]
    assert [s for m, s in ours["segments"] if m == 0xC4] == [s for m, s in theirs["segments"] if m == 0xC4]      # the very bytes
    assert ours["comps"] == [(1, 0x11, 0), (2, 0x11, 1), (3, 0x11, 1)] == theirs["comps"]
    assert ours["sos"] == [(1, 0, 0), (2, 1, 1), (3, 1, 1)] == theirs["sos"]
    assert ours["ri"] == MJ.limit(1) and (ours["H"], ours["W"]) == (16, 16)
    assert len(hdr) == MJ.limit(6) == ours["scan"]


@pytest.mark.parametrize("cid", MC.IDS)
def test_entropy_coding_loses_nothing(cid):
    c = MC.BY_ID[cid]
    for f, jpeg, (h, coefs, stats) in zip(c.frames, MC.host_files(cid), MC.decoded(cid)):
        assert (h["H"], h["W"]) == f.shape[:2] and len(jpeg) <= MJ.bound(*f.shape[:2])
        assert np.array_equal(coefs, MJ.coefficients_host(f, c.quality))
        M = coefs.shape[0]
        assert stats["intervals"] == (M + MJ.limit(1) - 1) // MJ.limit(1)


def test_the_matrix_fires():
    """A case that cannot fire tests nothing: the twin's files really contain what the matrix is there for."""
    total = sum((s for cid in MC.IDS for _, _, s in MC.decoded(cid)), collections.Counter())
    assert total["stuffed"] > 0 and total["zrl"] > 0 and total["eob"] > 0
    assert total[("ac", 10)] > 0 and total[("dc", 11)] > 0
    assert any(len(j) % 2 for cid in MC.IDS for j in MC.host_files(cid)) and any(len(j) % 2 == 0 for cid in MC.IDS for j in MC.host_files(cid))
    assert max(s["intervals"] for cid in MC.IDS for _, _, s in MC.decoded(cid)) > 8
    print({str(k): v for k, v in sorted(total.items(), key=str)})


@pytest.mark.parametrize("cid", MC.IDS)
def test_coefficients_against_the_float64_model(cid):
    """Never more than one quantisation step from the exactly rounded exact transform, and equal wherever the exact quotient is
    farther from a half-integer than E / q, E the bound derived in the header from its fixed-point widths."""
    c = MC.BY_ID[cid]
    E = MC.error_bound()
    assert E <= 0.53
    ql, qc, _ = MJ.tables(c.quality)
    step = np.stack([np.asarray(t, np.float64)[MC.ZZ] for t in (ql, qc, qc)])[None]
    for f in c.frames:
        got = MJ.coefficients_host(f, c.quality).astype(np.int64)
        quo = MC.model_quotients(f, ql, qc)
        exact = np.sign(quo) * np.floor(np.abs(quo) + 0.5)                       # round half away from zero
        exact[..., 1:] = np.clip(exact[..., 1:], -1023, 1023)                    # category 11 does not exist for AC
        frac = np.abs(quo) - np.floor(np.abs(quo))
        in_band = np.abs(frac - 0.5) <= E / step
        print(f"{cid}: {100 * in_band.mean():.2f}% of the coefficients inside the band of +-{E:.3f}/q around a half-integer")
        assert np.abs(got - exact).max() <= 1
        assert np.array_equal(got[~in_band], exact[~in_band])


def restart_allowance(jpeg) -> int:
    """Bytes the restart intervals may cost over a file without them: the DRI segment; per interval a marker, up to a byte of
    padding, and three DC values coded from zero rather than from their neighbour (at most 20 + 22 + 22 bits)."""
    h, _, stats = MC.decode_scan(jpeg)
    return 6 + stats["intervals"] * (2 + 1 + 8)


@pytest.mark.parametrize("cid", MC.IDS)
def test_pillow_opens_the_files_and_its_own_encoding_is_no_better(cid):
    c = MC.BY_ID[cid]
    ql, qc, _ = MJ.tables(c.quality)
    for f, jpeg in zip(c.frames, MC.host_files(cid)):
        H, W = f.shape[:2]
        im = Image.open(io.BytesIO(jpeg))
        assert im.format == "JPEG" and im.size == (W, H)
        ours = MC.psnr(MC.pillow_decode(jpeg), f)
        ref = MC.pillow_encode(f, ql, qc)
        theirs = MC.psnr(MC.pillow_decode(ref), f)
        print(f"{cid}: psnr {ours:.3f} dB, pillow {theirs:.3f} dB, shortfall {theirs - ours:+.3f}; bytes {len(jpeg)}, pillow {len(ref)}, "
              f"allowance {restart_allowance(jpeg)}")
        assert ours >= theirs - PSNR_MARGIN_DB
        assert len(jpeg) <= len(ref) + restart_allowance(jpeg)
