"""-m gpu: PNG files decoded on the device (include_ext/openglottal_hip_png.h).  The device gives the host twin's bytes AND statuses on
the whole valid set and the whole hostile corpus of tests/png_cases.py (one call each, mixed sizes, chunk 3, so that micro-batches
and pinned slots turn over), on the shapes that sit on the kernels' seams, resident and streamed, at C = 3 and C = 1; the ring
files and the errors beyond the first window are judged by the independent numpy decoder as well, and k_png_expand walks files larger
than its grid; `read_pairs` feeds `evaluate_device`, and `cli infer --mode images --decode device` writes what `--decode host` writes."""
import functools
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import png_cases as PC
from openglottal_amd import png as P
from openglottal_amd.utils import bgr_to_gray

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def decoder():
    return P.PngDecoder(chunk=3)


def twin(files, C=3):
    """[(pixels, status)] of the host twin; a refused file has shape (0, 0, C)"""
    out = []
    for f in files:
        px, st = P.decode_host(f, C, statuses=True)
        out.append((np.zeros((0, 0, C), np.uint8) if px is None else px, st))
    return out


def as_list(out):
    if isinstance(out, (list, tuple)):
        return [o.cpu().numpy() if hasattr(o, "cpu") else o for o in out]
    return list(out.cpu().numpy() if hasattr(out, "cpu") else out)


def hold_to_twin(d, files, C=3, resident=False):
    want = twin(files, C)
    got, st = (d.decode_resident if resident else d.decode)(files, C, statuses=True)
    got = as_list(got)
    assert st.tolist() == [s for _, s in want]
    assert len(got) == len(files)
    for i, (px, _) in enumerate(want):
        assert got[i].shape == px.shape and np.array_equal(got[i], px), (i, got[i].shape, px.shape)
    return got, st


@pytest.mark.parametrize("C", [3, 1])
def test_the_valid_set_in_one_call(decoder, C):
    files = [f for _, f in PC.valid_cases()]
    assert len(files) >= 8 and len({f[16:24] for f in files}) > 4              # mixed sizes
    _, st = hold_to_twin(decoder, files, C)
    assert not st.any()


def test_the_hostile_corpus_in_one_call(decoder):
    files = PC.hostile_corpus()
    got, st = hold_to_twin(decoder, files)
    assert set(st.tolist()) == set(range(8))
    assert all(not g.any() for g, s in zip(got, st) if s)


def seam_files():
    out = [PC.simple(H, 5, 2, 8, None, H) for H in (1, 63, 64, 65, 129)]                                   # the band carry
    out += [PC.simple(67, rb, 0, 8, None, rb) for rb in (1, 2, 63, 64, 65)]                               # rb
    out += [PC.simple(3, 5, ct, depth, None, depth) for ct in (0, 3) for depth in (1, 2, 4)]              # a partial last byte
    out += [PC.simple(66, 9, ct, 8, [4] * 66, ct) for ct in (0, 4, 2, 6)]                                 # bpp 1 2 3 4, Paeth across a band
    out += [PC.simple(66, 9, ct, 8, [3] * 66, ct) for ct in (0, 4, 2, 6)]                                 # Average
    out.append(PC.simple(130, 7, 2, 8, [2, 4] * 65, 9))                                                   # a row of Paeth after a row of Up
    return out


def test_shapes_on_the_seams(decoder):
    files = seam_files()
    for f in files:                                                           # (the twin itself against Pillow on these)
        assert np.array_equal(P.decode_host(f), PC.pillow(f))
    _, st = hold_to_twin(decoder, files)
    assert not st.any()
    hold_to_twin(decoder, files, 1, resident=True)


def test_one_match_at_distance_32768(decoder):
    f = dict(PC.valid_cases())["far-match-32768"]
    got, st = hold_to_twin(decoder, [f])
    assert not st.any() and np.array_equal(got[0], PC.pillow(f))


@functools.lru_cache(None)
def judge(f, C):
    """the independent decoder (zlib.decompress and the numpy unfilter), once per file and C: a change to the inline functions moves
    device and twin together, this one stays"""
    return PC.reference(f, C)


def ring_call():
    """the ring files and the other late files of the valid set, a small file of an odd number of raw bytes in front of each"""
    late = [f for _, f in PC.valid_cases()[75:]]
    files = [g for i, f in enumerate(late) for g in (PC.simple(1, 2 + 2 * i, 0, 8, None, i), f)]
    at = P.records_host(files)["recs"]["raw_offset"][1::2]
    assert len(late) == len(PC.ring_files()) + 5 and (at % 2).any() and len(set((at % 4).tolist())) > 2        # raw offsets off every alignment
    return files


@pytest.mark.parametrize("C", [3, 1])
def test_the_ring_files_in_one_call(decoder, C):
    """k_png_inflate's window -- stored blocks into the ring, copies across the wrap point, matches that overwrite their own source,
    short distances against the 64-lane turn, tables rebuilt in LDS (tests/test_png_host.py asserts that each file holds its seam) --
    streamed at chunk 3 and resident, against the twin and against the independent decoder"""
    files = ring_call()
    for resident in (False, True):
        got, st = hold_to_twin(decoder, files, C, resident)
        assert not st.any()
        for i, (g, f) in enumerate(zip(got, files)):
            assert np.array_equal(g, judge(f, C)), i


@pytest.mark.parametrize("C", [3, 1])
def test_errors_beyond_the_first_window_beside_valid_files(decoder, C):
    deep = PC.deep_errors()
    good = [PC.ring_files()["ring-tables"].file, PC.simple(9, 17, 2, 8, None, 1), PC.ring_files()["ring-stored-match"].file]
    files = [g for i, (_, f, _, _) in enumerate(deep) for g in (f, good[i % 3])]
    for resident in (False, True):
        got, st = hold_to_twin(decoder, files, C, resident)
        assert st.tolist() == [s for _, _, want, _ in deep for s in (want, 0)]
        for i, (g, f) in enumerate(zip(got, files)):
            assert (not g.any() and g.size) if i % 2 == 0 else np.array_equal(g, judge(f, C)), i


STRIDED = (1, 255, 256, 257, 437, 4355)


@pytest.mark.parametrize("C", [3, 1])
def test_expand_walks_files_larger_than_its_grid(decoder, C):
    """k_png_expand with max_pixels below the largest H * W: a grid of one or two workgroups per file walks every file in strides and
    gives the bytes of the true max_pixels, nothing outside the records' ranges"""
    pillow = dict(PC.valid_cases())
    files = [PC.simple(1, 1, 0, 8, None, 1), PC.simple(15, 17, 2, 8, None, 2), PC.simple(16, 16, 6, 8, None, 3), PC.simple(1, 257, 4, 8, None, 4),
             pillow["pillow-3-4-l6"], pillow["pillow-0-1-l6"], PC.simple(67, 65, 3, 8, None, 5)]
    B, gap, edge = len(files), 5, 64
    r = P.records_host(files, C)
    recs = r["recs"].copy()
    assert sorted({int(h) * int(w) for h, w in zip(recs["H"], recs["W"])}) == list(STRIDED) == sorted(STRIDED) and r["max_pixels"] == 4355
    assert {3} <= set(recs["ctype"].tolist()) and 1 in recs["depth"].tolist()
    recs["out_offset"] += gap * np.arange(B)
    cap = r["out_bytes"] + gap * B
    want = np.full(cap, 0x5A, np.uint8)
    for f, rec in zip(files, recs):
        px = judge(f, C).reshape(-1)
        want[rec["out_offset"]:rec["out_offset"] + px.size] = px
    decoder.set_palettes(r["pals"])
    dev = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda() for a in (r["zblob"], r["zoffsets"], recs)]
    for max_pixels in (r["max_pixels"], 1, 256, 257):
        whole = torch.full((edge + cap + edge,), 0x5A, dtype=torch.uint8, device="cuda")
        out = whole[edge:edge + cap]
        status = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        decoder.decode_dev(*dev, B, C, r["raw_bytes"], max_pixels, out, cap, status)
        decoder.sync()
        assert status.cpu().tolist() == [0] * B, max_pixels
        got = whole.cpu().numpy()
        assert (got[:edge] == 0x5A).all() and (got[edge + cap:] == 0x5A).all() and np.array_equal(got[edge:edge + cap], want), max_pixels


def realistic():
    y, x = np.mgrid[0:256, 0:256]
    rgb = np.stack([(128 + 100 * np.sin(x / 17.0) * np.cos(y / 23.0)), (x + y) / 2, 255 - y], -1).astype(np.uint8)
    rgb[60:200, 100:140] //= 3
    g = (np.hypot(np.mgrid[0:128, 0:512][0] - 64, (np.mgrid[0:128, 0:512][1] - 256) / 4) * 3).clip(0, 255).astype(np.uint8)
    a, b = io.BytesIO(), io.BytesIO()
    Image.fromarray(rgb).save(a, "PNG", compress_level=6)
    Image.fromarray(g, "L").save(b, "PNG", compress_level=6)
    return [a.getvalue(), b.getvalue()], [rgb[..., ::-1], np.repeat(g[..., None], 3, 2)]


def test_a_realistic_rgb_file_next_to_a_gray_one(decoder):
    files, want = realistic()
    got, st = hold_to_twin(decoder, files)
    assert not st.any() and all(np.array_equal(g, w) for g, w in zip(got, want))


def test_resident_and_streamed_agree_and_gray_is_bgr_to_gray(decoder):
    files = [f for _, f in PC.valid_cases()][:24] + realistic()[0]
    host = as_list(decoder.decode(files))
    res = decoder.decode_resident(files)
    assert all(isinstance(r, torch.Tensor) and r.is_cuda for r in res)
    gray = as_list(decoder.decode(files, 1))
    for h, r, g in zip(host, as_list(res), gray):
        assert np.array_equal(h, r) and np.array_equal(g[..., 0], bgr_to_gray(h))
    same = [files[0]] * 5
    out = decoder.decode_resident(same)                                       # sizes agree: one [B,H,W,C] tensor
    assert isinstance(out, torch.Tensor) and out.shape == (5, 23, 19, 3) and np.array_equal(out[4].cpu().numpy(), host[0])
    with pytest.raises(P.OpenGlottalHipError, match="status 5"):
        decoder.decode([files[0], dict((n, f) for n, f, _ in PC.hand_made_invalid())["adler"]])
    assert np.array_equal(decoder.decode([files[0]])[0], host[0])              # the handle stays usable


def test_the_resident_python_entry(decoder):
    files = [f for _, f in PC.valid_cases()][:9] + [b"junk"]
    r = P.records_host(files)
    decoder.set_palettes(r["pals"])
    dev = [torch.from_numpy(np.ascontiguousarray(r[k]).view(np.uint8).reshape(-1)).cuda() for k in ("zblob", "zoffsets", "recs")]
    out = torch.full((r["out_bytes"],), 0x5A, dtype=torch.uint8, device="cuda")
    status = torch.full((len(files),), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    decoder.decode_dev(*dev, len(files), 3, r["raw_bytes"], r["max_pixels"], out, out.numel(), status)
    decoder.sync()
    want = twin(files)
    assert status.cpu().tolist() == [s for _, s in want] == [0] * 9 + [6]
    assert np.array_equal(out.cpu().numpy(), np.concatenate([p.reshape(-1) for p, _ in want]))


def test_read_pairs_feeds_evaluate_device(tmp_path, golden_dir):
    import openglottal_amd as og
    from openglottal_amd import evaluate as E
    from openglottal_amd import synth

    g = np.load(os.path.join(golden_dir, "unet_trained_small.npz"))
    m = og.UNet(1, 1, tuple(int(f) for f in g["features"]))
    m.load_state_dict({k[2:]: g[k] for k in g.files if k.startswith("W:")})
    m.to("cuda:0").eval()
    frames, gts = synth.bagls_standin(12, seed=5)
    for i, (f, t) in enumerate(zip(frames, gts)):
        Image.fromarray(np.ascontiguousarray(np.asarray(f)[..., ::-1])).save(tmp_path / f"{i}.png")
        if i != 7:                                                            # a pair without a label is left out
            Image.fromarray(np.asarray(t), "L").save(tmp_path / f"{i}_seg.png")
    imgs, segs = P.bagls_pairs(str(tmp_path))
    assert [os.path.basename(p) for p in imgs] == [f"{i}.png" for i in sorted((i for i in range(12) if i != 7), key=str)]
    assert len(P.bagls_pairs(str(tmp_path), 3)[0]) == 3
    got_f, got_g = P.read_pairs(imgs, segs)
    pil_f = [np.ascontiguousarray(np.asarray(Image.open(p).convert("RGB"))[..., ::-1]) for p in imgs]
    pil_g = [np.asarray(Image.open(p).convert("L")) for p in segs]
    assert all(np.array_equal(a, b) for a, b in zip(got_f, pil_f)) and all(np.array_equal(a, b) for a, b in zip(got_g, pil_g))
    agg_d, st_d = E.evaluate_device(got_f, got_g, m)
    agg_p, st_p = E.evaluate_device(pil_f, pil_g, m)
    assert agg_d == agg_p and st_d == st_p and agg_d["unet-only"]["n_total"] == 11


def test_cli_infer_decodes_a_png_directory_on_the_device(tmp_path, capsys):
    from openglottal_amd import cli, synth

    feats = (32, 64, 128, 256)
    torch.save(synth.state_dict_to_torch(synth.make_unet_state_dict(feats, seed=5, head_scale=3.0, head_bias=-2.5)), tmp_path / "unet.pt")
    os.makedirs(tmp_path / "seq")
    rs = np.random.RandomState(3)
    for i in range(6):
        Image.fromarray((rs.randint(0, 256, (64, 64, 3)) // 2 + 40).astype(np.uint8)).save(tmp_path / "seq" / f"{i:03d}.png")
    base = ["infer", "--input", str(tmp_path / "seq"), "--mode", "images", "--pipeline", "unet-only", "--unet-weights", str(tmp_path / "unet.pt")]
    for d in ("host", "device", "auto"):
        assert cli.main(base + ["--output-dir", str(tmp_path / d), "--decode", d]) == 0
    assert "--decode auto" not in capsys.readouterr().err
    for d in ("device", "auto"):
        assert sorted(os.listdir(tmp_path / d)) == sorted(os.listdir(tmp_path / "host")) == ["features.csv", "seq_out.npy"]
        assert open(tmp_path / d / "features.csv").read() == open(tmp_path / "host" / "features.csv").read()
        assert np.array_equal(np.load(tmp_path / d / "seq_out.npy"), np.load(tmp_path / "host" / "seq_out.npy"))
    assert np.load(tmp_path / "host" / "seq_out.npy").shape == (6, 64, 64, 3)
