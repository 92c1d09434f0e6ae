"""og_png_plan: the dry run of the streamed PNG decode records the launches the product's own batch function would make -- three per
micro-batch, grids from the files' shapes, static LDS stated, writes inside the caller's buffers -- and the micro-batches are cut by
`chunk` and by 256 MiB of raw bytes.  No GPU."""
import pytest

from openglottal_amd import png as P
from openglottal_amd._lib import OpenGlottalHipError

BAGLS = [(256, 256, 2, 8), (512, 256, 2, 8), (512, 128, 0, 8), (352, 208, 3, 8)]


def raw(f):
    H, W, ct, d = f
    return H * (1 + (W * {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ct] * d + 7) // 8)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("chunk", [1, 3, 128])
def test_launches_grids_and_writes(chunk, C):
    forms = BAGLS * 2 + [(1, 1, 0, 1)]
    recs, ws = P.plan(forms, C, chunk)
    B = len(forms)
    nbatch = -(-B // chunk)
    assert [r["kernel"] for r in recs] == ["k_png_inflate", "k_png_unfilter", "k_png_expand"] * nbatch
    done, out_end, ws_max = 0, 0, 0
    for k in range(nbatch):
        part = forms[done:done + chunk]
        nb = len(part)
        inf, unf, exp = recs[3 * k:3 * k + 3]
        assert (inf["gx"], inf["gy"], inf["gz"], inf["block"], inf["lds"]) == (nb, 1, 1, 64, 32768 + 1056)      # a wave per file
        assert (unf["gx"], unf["gy"], unf["gz"], unf["block"], unf["lds"]) == (nb, 1, 1, 64, 0)
        assert (exp["gx"], exp["gy"], exp["gz"], exp["block"]) == (-(-max(f[0] * f[1] for f in part) // 256), nb, 1, 256)
        done += nb
        out_end += sum(f[0] * f[1] * C for f in part)
        need = (sum(raw(f) for f in part) + 3) // 4 * 4 + 4 * nb
        assert inf["workspace"] == need and unf["workspace"] == exp["workspace"] == 0
        ws_max = max(ws_max, need)
        assert inf["writes"] == unf["writes"] == f"status={4 * done}" and exp["writes"] == f"out={out_end}"
        assert inf["lds"] <= 64 << 10 and exp["gx"] <= 65536 and exp["gy"] <= 65535
    assert ws >= ws_max + max(f[0] * f[1] * C for f in forms)


def test_a_micro_batch_is_cut_at_256_mib_of_raw_bytes():
    big = (4096, 4096, 6, 8)                                                  # 64 MiB of raw bytes each
    recs, _ = P.plan([big] * 9, 3, 128)
    assert [r["gx"] for r in recs if r["kernel"] == "k_png_inflate"] == [3, 3, 3]
    recs, _ = P.plan([(4096, 4096, 6, 8), (1, 1, 0, 8)] * 2, 1, 128)
    assert [r["gx"] for r in recs if r["kernel"] == "k_png_inflate"] == [4]


def test_refusals():
    for forms, C, chunk in (([(0, 4, 0, 8)], 3, 1), ([(4, 4, 2, 4)], 3, 1), ([(4, 4, 0, 16)], 3, 1), ([(4, 4, 0, 8)], 2, 1), ([(4, 4, 0, 8)], 3, 0),
                            ([(4, 4, 0, 8)], 3, 1025), ([(4097, 4096, 0, 8)], 3, 1), ([], 3, 1)):
        with pytest.raises(OpenGlottalHipError):
            P.plan(forms, C, chunk)
    assert P.PngDecoder(chunk=5).plan(BAGLS)[0][0]["gx"] == 4
