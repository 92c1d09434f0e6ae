"""The rules tests/test_pnge_abi.py holds the thirteenth header to, on the fourteenth, include_enc/openglottal_hip_aug.h: every function
it declares is exported and bound (`_lib.AUG_PROTOTYPES`) and vice versa, the table is disjoint from the thirteen older ones and those
keep their sizes, every argument and alignment check comes before the first HIP call, and b = 0 is a no-op.  No GPU."""
import os

import numpy as np

from openglottal_amd import _lib
from openglottal_amd import augment as A
from openglottal_amd._lib import lib
from test_mjpd_abi import OLDER, ROOT, _declarations

OG_EINVAL = -1
HEADER = os.path.join(ROOT, "include_enc", "openglottal_hip_aug.h")
NAMES = {"og_aug_limit", "og_aug_stage_host", "og_aug_apply_host", "og_aug_noise_host", "og_aug_create", "og_aug_destroy", "og_aug_sync",
         "og_aug_set_chunk", "og_aug_batch_u8_dev", "og_aug_plan"}


def test_every_function_of_the_header_is_exported_and_bound_and_vice_versa():
    decl = _declarations(HEADER)
    assert set(decl) == NAMES == set(_lib.AUG_PROTOTYPES)
    l = lib()
    for name in sorted(decl):
        assert hasattr(l, name), f"{name} declared in the header but not exported"
        args = _lib.AUG_PROTOTYPES[name][1]
        assert list(getattr(l, name).argtypes or []) == args, name
        assert len(args) == (0 if decl[name] == ["void"] else len(decl[name])), name
    text = open(HEADER).read()
    assert '#include "openglottal_hip_pnge.h"' in text and "UNPINNED" in text and "OUT OF SCOPE" in text
    for word in ("antialias", "randn", "training loop", "multi-channel", "non-square", "expand=True", "torchvision parity"):
        assert word in text, word


def test_the_thirteen_older_tables_keep_their_sizes():
    seen = set(_lib.AUG_PROTOTYPES)
    older = dict(OLDER, **{"decode/openglottal_hip_mjpd.h": ("MJPD_PROTOTYPES", 13), "split/openglottal_hip_mjps.h": ("MJPS_PROTOTYPES", 4)})
    for header, (table, count) in older.items():
        t = getattr(_lib, table)
        assert len(t) == count and set(_declarations(os.path.join(ROOT, "include", header))) == set(t), header
        assert not (set(t) & seen), header
        seen |= set(t)
    for table, count, path in (("PNG_PROTOTYPES", 13, "include_ext/openglottal_hip_png.h"), ("PNGE_PROTOTYPES", 16, "include_enc/openglottal_hip_pnge.h")):
        t = getattr(_lib, table)
        assert len(t) == count and not (set(t) & seen) and set(_declarations(os.path.join(ROOT, path))) == set(t), table
        seen |= set(t)
    api = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_api.hip")).read()
    assert api.count('#include "og_aug.inc"') == 1 and api.index('#include "og_pnge.inc"') < api.index('#include "og_aug.inc"')
    src = open(os.path.join(ROOT, "openglottal_amd", "csrc", "og_aug.inc")).read()
    assert "asm" not in src and all(k in src for k in ("k_aug_rotate", "k_aug_scale", "k_aug_blur", "k_aug_contrast", "OG_PNG_HOST_ONLY"))
    assert src.count("#pragma clang fp contract(off)") >= 9
    for word in ("expf", "logf", "cosf", "sinf", "powf", "__expf", "__logf"):  # no transcendental function on the device
        assert word + "(" not in src, word
    assert "openglottal_hip_aug.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_limits_and_the_record():
    l = lib()
    assert [l.og_aug_limit(i) for i in range(8)] == [8, 1024, 1024, 128, 2, 64, 1024, 8]
    assert l.og_aug_limit(8) == -1 and l.og_aug_limit(-1) == -1
    assert A.PARAMS.itemsize == 64
    assert {n: A.PARAMS.fields[n][1] for n in A.PARAMS.names} == {"flips": 0, "cos_t": 4, "sin_t": 8, "new_size": 12, "noise_sigma": 16, "ks": 20,
                                                                 "noise_key": 24, "k1": 32, "brightness": 52, "contrast": 56, "reserved": 60}


def test_the_handle_refuses_bad_arguments_without_a_device():
    """Argument checks come before the first HIP call, so they can be held here."""
    l = lib()
    h = l.og_aug_create()
    assert h
    try:
        raw = np.zeros(1 << 16, np.uint8)
        base = raw.ctypes.data + (-raw.ctypes.data) % 8
        images, masks, idx, par, oi, om = (base + 8192 * i for i in range(6))
        recs = np.frombuffer(raw, A.PARAMS, 2, par - raw.ctypes.data)
        recs[:] = A.records([A.record(angle=30, new_size=36), A.record(ks=3, blur_sigma=1.0)])
        before = raw.copy()
        f, N, S, b = l.og_aug_batch_u8_dev, 3, 32, 2
        assert f(None, images, masks, N, S, idx, par, b, 1, oi, om) == OG_EINVAL and b"null handle" in l.og_last_error()
        for bad_S in (0, 7, 1025, -32):
            assert f(h, images, masks, N, bad_S, idx, par, b, 1, oi, om) == OG_EINVAL and b"S must be 8..1024" in l.og_last_error()
        assert f(h, images, masks, 0, S, idx, par, b, 1, oi, om) == OG_EINVAL and f(h, images, masks, N, S, idx, par, -1, 1, oi, om) == OG_EINVAL
        for off in (1, 2, 3):
            assert f(h, images, masks, N, S, idx + off, par, b, 1, oi, om) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
            assert f(h, images, masks, N, S, idx, par, b, 1, oi + off, om) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
            assert f(h, images, masks, N, S, idx, par, b, 1, oi, om + off) == OG_EINVAL and b"aligned to 4" in l.og_last_error()
        for off in (1, 2, 4):
            assert f(h, images, masks, N, S, idx, par + off, b, 1, oi, om) == OG_EINVAL and b"aligned to 8" in l.og_last_error()
        for i in (0, 1, 4, 5, 8, 9):
            args = [images, masks, N, S, idx, par, b, 1, oi, om]
            args[i] = None
            assert f(h, *args) == OG_EINVAL and b"null buffer" in l.og_last_error(), i
        for field, value, why in (("new_size", 15, b"new_size"), ("new_size", 65, b"new_size"), ("ks", 4, b"ks must be"), ("flips", 4, b"flips"),
                                  ("cos_t", 1.5, b"cos_t"), ("sin_t", np.nan, b"cos_t"), ("noise_sigma", -0.1, b"noise_sigma"),
                                  ("brightness", np.inf, b"brightness"), ("contrast", -1, b"contrast")):
            keep = recs[field][1]
            recs[field][1] = value
            assert f(h, images, masks, N, S, idx, par, b, 1, oi, om) == OG_EINVAL, field
            assert why in l.og_last_error() and b"record 1" in l.og_last_error(), field
            recs[field][1] = keep
        assert f(h, images, masks, N, S, idx, par, 0, 1, oi, om) == 0 and f(h, None, None, N, S, None, None, 0, 0, None, None) == 0     # b = 0
        assert np.array_equal(raw, before)                                    # nothing touched a device or a buffer
        assert l.og_aug_set_chunk(h, 0) == OG_EINVAL and l.og_aug_set_chunk(h, 1025) == OG_EINVAL and l.og_aug_set_chunk(h, 7) == 0
        assert l.og_aug_set_chunk(None, 4) == OG_EINVAL and l.og_aug_sync(None) == OG_EINVAL
        assert l.og_aug_sync(h) == 0                                          # no stream yet: nothing to wait for
    finally:
        l.og_aug_destroy(h)
    l.og_aug_destroy(None)


def test_the_host_entries_refuse_bad_arguments_and_write_nothing():
    l = lib()
    S = 8
    I, M = np.full((S, S), 0.5, np.float32), np.ones((S, S), np.uint8)
    oi, om, of = np.zeros((S, S), np.float32), np.zeros((S, S), np.uint8), np.zeros((S, S), np.float32)
    r = A.records([A.record(angle=5)])
    st, ap, no = l.og_aug_stage_host, l.og_aug_apply_host, l.og_aug_noise_host
    p = lambda a: a.ctypes.data                                               # noqa: E731
    for stage in (0, 8, -1):
        assert st(stage, p(I), p(M), S, p(r), p(oi), p(om)) == OG_EINVAL and b"stage must be 1..7" in l.og_last_error()
    assert st(2, p(I), p(M), 7, p(r), p(oi), p(om)) == OG_EINVAL and st(2, None, p(M), S, p(r), p(oi), p(om)) == OG_EINVAL
    assert st(2, p(I), p(M), S, None, p(oi), p(om)) == OG_EINVAL and st(2, p(I), p(M), S, p(r), None, p(om)) == OG_EINVAL
    assert st(2, p(I), p(M), S, p(r), p(oi), None) == OG_EINVAL and st(2, p(I), None, S, p(r), p(oi), p(om)) == OG_EINVAL      # half a mask
    assert st(2, p(I) + 2, p(M), S, p(r), p(oi), p(om)) == OG_EINVAL and st(2, p(I), p(M), S, p(r) + 4, p(oi), p(om)) == OG_EINVAL
    bad = r.copy()
    bad["ks"] = 7
    assert st(5, p(I), p(M), S, p(bad), p(oi), p(om)) == OG_EINVAL and ap(p(M), p(M), S, p(bad), 1, p(oi), p(of)) == OG_EINVAL
    assert ap(None, p(M), S, p(r), 1, p(oi), p(of)) == OG_EINVAL and ap(p(M), p(M), S, None, 1, p(oi), p(of)) == OG_EINVAL
    assert ap(p(M), p(M), 1025, p(r), 1, p(oi), p(of)) == OG_EINVAL and ap(p(M), p(M), S, p(r), 1, p(oi) + 1, p(of)) == OG_EINVAL
    assert no(1, 4, None) == OG_EINVAL and no(1, 4, p(oi) + 2) == OG_EINVAL and no(1, 0, None) == 0
    assert not oi.any() and not om.any() and not of.any()
    assert st(2, p(I), None, S, p(r), p(oi), None) == 0 and oi.any()          # no mask at all is fine
    assert ap(p(M), p(M), S, None, 0, p(oi), p(of)) == 0 and np.array_equal(oi, M / np.float32(255.0)) and (of == 1).all()
