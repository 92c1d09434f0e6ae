"""CPU (needs hipcc): the gfx950 code of every k_conv_mfma_f instantiation (f16 mode) has no scratch, runs the f16 MFMA and never
the f32 one."""
import os
import re

import pytest

import isa_listing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_f16_conv_kernels_have_no_scratch_and_use_the_f16_mfma():
    with open(isa_listing.listing()) as f:     # compiled once for all tests/test_isa_*.py modules
        s = f.read()
    names = sorted(set(re.findall(r"^(_Z13k_conv_mfma_fI\w+):", s, re.M)))
    assert len(names) == 7, names          # <1,0,8,FIRST> <2,0,16> <2,0,16,SQ> <1,0,16> <2,0,8> <1,0,8> <2,1,8>
    for n in names:
        body = s[s.index("\n" + n + ":"):]
        body = body[:body.index(".Lfunc_end")]
        assert "v_mfma_f32_32x32x16_f16" in body and "v_mfma_f32_32x32x2_f32" not in body, n
        assert "scratch_" not in body, n
        desc = s[s.index(".amdhsa_kernel " + n):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", desc), n
        meta = re.search(r"\.name:\s+" + re.escape(n) + r"\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", s)
        assert meta and int(meta.group(1)) == 0, n
