"""Static guard on the chunk loop of k_conv_wino<1> and <2> (no GPU needed: hipcc cross-compiles).

The Winograd kernels run ONE wave per SIMD (256 accumulator registers), so nothing but the wave's own instruction stream fills
the shadow of its MFMAs, and every other instruction between two MFMAs takes issue time from the matrix pipe.  Until this guard
the loop tested a run-time `nxt` in every fenced slot (51 branches, 19 v_cndmask and 155 scalar instructions per chunk of <2>,
one MFMA gap of 32 instructions) and saved / restored M0 around every LDS-DMA.  The chunk body is now instantiated on a
compile-time NXT and the last chunk peeled (og_kernels.hpp, k_conv_wino); this test compiles the device code to assembly, runs
tools/isa_wino_loop.py on it and checks, for both instantiations, in the steady-state body (the loop that holds 64 * NT MFMAs):
  * 64 * NT MFMAs; at most 3 branches (back edge + loop exit; a rotated loop may have two back edges), none of them jumping to
    a label inside the body (= guarding a DMA, a V write or a transform micro-op);
  * vector-ALU instructions = the 64 v_pk_add_f32 of the transform and nothing else;
  * no instruction reads M0; writes of M0 = LDS-DMA count (22 | 9);
  * scalar ALU + s_nop <= 3 per LDS-DMA + 8: per transfer one write of M0, the wait state, at most one s_add for an SGPR offset
    that does not fit the 12-bit immediate; 8 for loop control and the running offsets of the two DMA streams;
  * largest MFMA gap <= 12 instructions.  A construction bound: the fullest slot of the source holds eight packed adds (<1>), or
    one DMA group (<= 4 instructions) + four micro-ops (<2>), each plus at most one s_waitcnt = 9, + the loop-control instructions
    at the two ends of the body.  If hipcc piles more into one gap, the source is to be fixed, not the bound;
  * no scratch, and VGPR / AGPR counts not above those of the loop with run-time guards (226 / 256 for <1>, 231 / 256 for <2>):
    the register budget the design rests on (one wave per SIMD, nothing spilled) is unchanged;
  * in the whole kernel no LDS-DMA is directly followed by an instruction that writes one of its operand registers: the transfers
    of the loop carry no pad behind them (glds16b_m0<false>, og_kernels.hpp), which is only sound while that holds;
and in the peeled last chunk: 64 * NT MFMAs, no LDS-DMA in its second group, no transform (no vector ALU at all).
"""
import json
import os
import subprocess
import sys

import pytest

import isa_listing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

DMA = {2: 22, 1: 9}
VGPR_MAX = {2: 231, 1: 226}
GAP_MAX = 12


@pytest.fixture(scope="module")
def rows():
    asm = isa_listing.listing()     # compiled once for all tests/test_isa_*.py modules
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_wino_loop.py"), str(asm), "--json"],
                         check=True, capture_output=True, text=True).stdout
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_wino_loop.py"), str(asm)],
                         check=True, capture_output=True, text=True).stdout
    print(txt)
    return {int(r["kernel"][-2]): r for r in json.loads(out)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("nt", [2, 1])
def test_steady_state_chunk_is_branch_free_and_select_free(rows, nt):
    r = rows[nt]
    assert r["loop_found"], r
    b = r["body"]
    assert b["mfma"] == 64 * nt, r
    assert r["mfma_before_loop"] == 0, r
    assert b["branch"] <= 3 and r["guard_branches"] == 0, r
    assert b["v_pk_add"] == 64 and b["valu"] == 0, r
    assert b["dma"] == DMA[nt], r
    assert r["m0_reads"] == 0 and r["m0_writes"] == b["dma"], r
    assert b["salu"] + b["s_nop"] <= 3 * b["dma"] + 8, r
    assert max(r["gap_max"], r["gap_tail"] + r["gap_head"]) <= GAP_MAX, r     # (tail + head = the gap across the back edge)
    assert r["dma_operand_overwritten_next"] == 0, r
    assert r["scratch"] == 0 and r["vgprs"] <= VGPR_MAX[nt] and r["agprs"] <= 256, r


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("nt", [2, 1])
def test_last_chunk_is_peeled_without_transform_and_next_dma(rows, nt):
    r = rows[nt]
    assert r["loop_found"], r
    p = r["peel"]
    assert p["mfma"] == 64 * nt, r
    assert p["dma_second_group"] == 0, r
    assert p["v_pk_add"] == 0 and p["valu"] == 0, r
    assert p["ds_write"] == 8, r          # the hi half of the last chunk's V, nothing of a next chunk
