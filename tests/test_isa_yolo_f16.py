"""CPU (needs hipcc): the gfx950 code of every k_conv_mfma_fy instantiation (the detector's f16 mode) has no scratch, runs the f16
MFMA and never the f32 one.  The store-hazard scan (every 16-byte buffer store of the build, the new epilogue's included) finds
nothing; tools/isa_audit.py counts vector-ALU instructions in the MFMA blocks of `k_conv_mfma_o` only, so its run here shows that
the untouched f32 kernels still pass on this build, and says nothing about `k_conv_mfma_fy`."""
import os
import re
import subprocess
import sys

import pytest

import isa_listing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_detector_f16_conv_kernels_have_no_scratch_and_use_the_f16_mfma():
    asm = isa_listing.listing()     # compiled once for all tests/test_isa_*.py modules
    with open(asm) as f:
        s = f.read()
    names = sorted(set(re.findall(r"^(_Z14k_conv_mfma_fyI\w+):", s, re.M)))
    assert len(names) == 8, names   # <1|2, MODE 0> <1|2, MODE 2> <1|2, MODE 2, F32OUT> <1|2, MODE 3>
    for n in names + ["_Z17k_conv_direct_u8hPKhiiPKfS2_S2_iPfxiiiiiiiiiiPi", "_Z12k_maxpool5_hPKfPfxiiiiiix"]:
        assert "\n" + n + ":" in s, n
        body = s[s.index("\n" + n + ":"):]
        body = body[:body.index(".Lfunc_end")]
        if n in names:
            assert "v_mfma_f32_32x32x16_f16" in body and "v_mfma_f32_32x32x2_f32" not in body, n
        assert "scratch_" not in body, n
        desc = s[s.index(".amdhsa_kernel " + n):]
        desc = desc[:desc.index(".end_amdhsa_kernel")]
        assert re.search(r"\.amdhsa_private_segment_fixed_size\s+0\b", desc), n
    audit = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_audit.py"), str(asm)], capture_output=True, text=True)
    assert audit.returncode == 0, audit.stdout + audit.stderr
    hz = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_store_hazard.py"), str(asm)], capture_output=True, text=True)
    assert hz.returncode == 0 and "overwritten by the next instruction: 0" in hz.stdout, hz.stdout
