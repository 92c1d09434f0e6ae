"""CPU: the resized-frame path (og_unet_stream_resized_u8 / og_unet_segment_resized_u8_dev) without a device.

* the INTER_LINEAR tap rule both resize kernels use (og_linear_taps_host runs the kernels' own function on the host) against
  geometry._linear_taps, the restatement the fixtures and the numpy path use;
* every launch of a resized call (og_unet_plan_resized) inside the library's limits, and every write into a caller-owned buffer
  inside that buffer -- the class of the round-4 fault (a write past the caller's `area`);
* argument errors;
* the generated code of k_resize_out's interpolation has no fused multiply-add (numpy rounds the products and sums separately).
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from openglottal_amd import geometry
from openglottal_amd._lib import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FULL = (32, 64, 128, 256)
SIZES = [(512, 512), (480, 640), (200, 100), (255, 257), (256, 320), (1080, 1920)]


def taps_host(src, dst):
    i0, i1, a1 = (np.empty(dst, np.int32) for _ in range(3))
    frac = np.empty(dst, np.float32)
    rc = lib().og_linear_taps_host(src, dst, i0.ctypes.data, i1.ctypes.data, frac.ctypes.data, a1.ctypes.data)
    assert rc == 0
    return i0, i1, frac, a1


LENS = [1, 2, 3, 7, 100, 200, 255, 256, 257, 320, 480, 512, 640, 1080, 1920, 4096]


@pytest.mark.parametrize("src", LENS)
def test_linear_taps_equal_the_numpy_restatement(src):
    for dst in LENS:
        i0, i1, frac, a1 = taps_host(src, dst)
        r0, r1, rf = geometry._linear_taps(dst, src)
        assert np.array_equal(i0, r0) and np.array_equal(i1, r1), (src, dst)
        assert np.array_equal(frac.view(np.int32), rf.view(np.int32)), (src, dst)   # bit for bit
        assert np.array_equal(a1, np.rint(rf * 2048).astype(np.int32)), (src, dst)
        if src == dst:   # an identity axis: exact taps
            assert not frac.any() and np.array_equal(i0, np.arange(dst))


def test_linear_taps_reject_bad_lengths():
    buf = np.empty(4, np.int32)
    f = np.empty(4, np.float32)
    for s, d in ((0, 4), (4, 0), (-1, 4)):
        assert lib().og_linear_taps_host(s, d, buf.ctypes.data, buf.ctypes.data, f.ctypes.data, buf.ctypes.data) == -1


def plan_resized(B, H, W, ch, net=(256, 256), lanes=1, options="", feats=FULL):
    l = lib()
    f = (C.c_int * len(feats))(*feats)
    buf = C.create_string_buffer(1 << 20)
    arena = C.c_longlong(0)
    n = l.og_unet_plan_resized(f, len(feats), B, H, W, ch, net[0], net[1], lanes, options.encode(), buf, len(buf), C.byref(arena))
    if n < 0:
        return n, None
    recs = []
    for line in buf.value.decode().strip().split("\n"):
        k, gx, gy, gz, blk, lds, ws, cnt, writes = line.rsplit("|", 8)
        w = {} if writes == "-" else {kv.split("=")[0]: int(kv.split("=")[1]) for kv in writes.split(";")}
        recs.append(dict(kernel=k, grid=(int(gx), int(gy), int(gz)), block=int(blk), lds=int(lds), ws=int(ws), cnt=int(cnt), writes=w))
    assert len(recs) == n
    return n, recs


@pytest.mark.parametrize("H,W", SIZES)
def test_resized_plan_stays_inside_limits_and_caller_buffers(H, W):
    l = lib()
    ws_max, cnt_max, g_max, lds_max = (l.og_workspace_limit(i) for i in range(4))
    for ch in (1, 3):
        for B in range(1, 65):
            n, recs = plan_resized(B, H, W, ch)
            assert n > 0, (H, W, ch, B, l.og_last_error())
            limit = {"mask": B * H * W, "area": 4 * B, "net_logits": 4 * B * 256 * 256, "net_prob": 4 * B * 256 * 256,
                     "prob": 4 * B * H * W}
            seen = {k: 0 for k in limit}
            for r in recs:
                gx, gy, gz = r["grid"]
                assert gx >= 1 and gy >= 1 and gz >= 1 and gy <= g_max and gz <= g_max and gx < 2 ** 31, (H, W, B, r)
                assert r["block"] == 256 and r["lds"] <= lds_max and r["ws"] <= ws_max and r["cnt"] <= cnt_max, (H, W, B, r)
                for k, end in r["writes"].items():
                    assert 0 < end <= limit[k], (H, W, ch, B, r)
                    seen[k] = max(seen[k], end)
            assert seen == limit, (H, W, ch, B, seen)   # and every frame's outputs are written
            kinds = [r["kernel"] for r in recs]
            assert sum(k.startswith("k_resize_in") for k in kinds) == sum(k == "k_resize_out" for k in kinds) >= 1


def test_resized_plan_lowers_the_micro_batch_for_large_frames():
    """1080 x 1920 BGR: 64 MiB of source frames per micro-batch -> 10 frames per chain, not the handle's 32."""
    _, recs = plan_resized(64, 1080, 1920, 3)
    ins = [r for r in recs if r["kernel"].startswith("k_resize_in")]
    assert [r["grid"][1] for r in ins] == [10] * 6 + [4]
    _, recs = plan_resized(64, 480, 640, 1)
    assert [r["grid"][1] for r in recs if r["kernel"].startswith("k_resize_in")] == [32, 32]


def test_resized_plan_at_network_size_is_the_existing_chain():
    """A frame already at the network size: no resize launch in front of the chain, the chain's head writes mask / area."""
    _, recs = plan_resized(8, 256, 256, 1)
    kinds = [r["kernel"] for r in recs]
    assert not any(k.startswith("k_resize_in") for k in kinds)
    assert any("mask" in r["writes"] and "area" in r["writes"] for r in recs)


@pytest.mark.parametrize("args", [
    dict(H=0), dict(W=-3), dict(net=(0, 256)), dict(net=(256, -256)), dict(net=(250, 256)), dict(net=(256, 264)),
    dict(ch=2), dict(ch=4), dict(H=8193), dict(W=10000), dict(B=0, H=0)])
def test_resized_plan_rejects_bad_arguments(args):
    a = dict(B=1, H=480, W=640, ch=1, net=(256, 256))
    a.update(args)
    n, _ = plan_resized(max(1, a["B"]), a["H"], a["W"], a["ch"], a["net"])
    assert n == -1


def test_resized_entries_reject_bad_arguments_without_a_handle_or_device():
    l = lib()
    fr = np.zeros((1, 8, 8), np.uint8)
    area = np.zeros(1, np.int32)
    assert l.og_unet_stream_resized_u8(None, fr.ctypes.data, 1, 8, 8, 1, 256, 256, 0.5, None, None, area.ctypes.data) == -1
    assert l.og_unet_stream_frames_resized_u8(None, None, 1, 8, 8, 1, 256, 256, 0.5, None, None, area.ctypes.data) == -1
    assert l.og_unet_segment_resized_u8_dev(None, None, 1, 8, 8, 1, 256, 256, 0.5, None, None, None, None, None, None) == -1


def test_resized_calls_need_a_finalized_handle():
    f = (C.c_int * 4)(*FULL)
    l = lib()
    h = l.og_unet_create(f, 4, 1, 1)
    assert h
    try:
        fr = np.zeros((1, 8, 8), np.uint8)
        area = np.zeros(1, np.int32)
        assert l.og_unet_stream_resized_u8(h, fr.ctypes.data, 1, 8, 8, 1, 256, 256, 0.5, None, None, area.ctypes.data) == -2
    finally:
        l.og_unet_destroy(h)


def _asm_function(asm, name_re):
    m = re.search(r"^(" + name_re + r"):[ \t]*(;.*)?$", asm, re.M)
    assert m, name_re
    body = asm[m.end():]
    return body[:body.index(".Lfunc_end")]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_resize_out_interpolation_has_no_fused_multiply_add(tmp_path):
    asm = tmp_path / "og_api.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    os.path.join(ROOT, "openglottal_amd", "csrc", "og_api.hip"), "-o", str(asm)],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    s = asm.read_text()
    lerp = _asm_function(s, r"_Z\d+og_resize_lerpffffff")
    assert re.search(r"\bv_(pk_)?mul_f32", lerp) and re.search(r"\bv_(pk_)?(add|sub)_f32", lerp), lerp
    bad = re.findall(r"\b(v_fma\w*|v_fmac\w*|v_mad\w*|v_pk_fma\w*)", lerp)
    assert not bad, bad
    out = _asm_function(s, r"_Z12k_resize_out\w*")
    assert "og_resize_lerp" in out   # the kernel interpolates through the audited function
    # the tap positions: ((d + 0.5) * scale) - 0.5 in two roundings, as numpy does (no v_fma_f64 outside the f64 division)
    for k in ("_Z11k_resize_inILi1EEvPKhiiiiPh", "_Z11k_resize_inILi3EEvPKhiiiiPh"):
        body = _asm_function(s, k)
        assert body.count("v_mul_f64") >= 2, k
