"""Static guard on the tile end of k_conv_wino<1> and <2> (no GPU needed: hipcc cross-compiles).

The Winograd kernels run ONE wave per SIMD and nothing overlaps the end of a tile, so every instruction behind the last MFMA is
paid in full, 212 times per CU and 64-frame chain.  The output transform Y = A^T M A runs on the register pairs the accumulators
already form -- (r, r + 1) of a slot = one window element of sub-tiles m and m + 1 -- and wino_tile_end consumes those pairs as they
stand, two sub-tiles per step, in one of 4 (<2>: ACT x POOL) or 12 (<1>: ACT x POOL x HEAD {none, fused head, fused head + stored
activation}) straight-line copies chosen once per tile.  This test compiles the two kernels to assembly (a translation unit of
its own that includes og_kernels.hpp and instantiates them: the same source and flags as the library, a tenth of the compile
time), runs tools/isa_wino_tail.py on it and checks, in the region behind the last MFMA of each instantiation:

  * v_accvgpr_read_b32 = 256: every accumulator register is read once;
  * v_pk_add_f32 of the transform = 192 exactly (24 packed adds per register pair x 8 pairs = the 384 additions of the transform; the
    parent issued 256), and in the whole region <= 192 + what the copies may add: wino_tile_end has no float addition but the fused
    head's (per sub-tile 4 row groups x 3 shuffle-reduction adds + the bias; hipcc issues them as v_add_f32 today, and if it ever
    packed the 12 pairwise that would be 6 per sub-tile = 24 per head copy): 0 for <2>, 8 head copies x 24 = 192 for <1>;
  * v_mov_b32: none that copies a VGPR (the parent had 220 | 226 of them: pairing registers up for its own packing), and in all
    no more than the constants the source sets up once per tile: one zero address per diagnostic stamp behind the loop (st[4..7])
    = 4, and per head copy the box defaults (4) and the "no detection" zeros (4), the out-of-range lane offset, the address and
    value of the per-wave count, and the mask / offset constants of a step (2) = 13: 4 for <2>, 4 + 8 x 13 = 108 for <1>
    (parent: 225 | 269);
  * s_mul_i32 <= the multiplications of the once-per-tile set-up, summed over the copies (a tile runs one copy): per copy 6 for
    the activation stream (frame base 3, first offset 2, row step 1), 6 more with a pooled stream, 14 with the head (frame offset of
    logits / mask 6, H W 1, count slot 7); a head copy that does not store the activation drops the first 6.  <2>: 2 x 6 + 2 x 12
    = 36; <1>: 36 + (4 x 14 + 2 x 6) + (4 x 20 + 2 x 6) = 196.  The parent had 41 | 107 in TWO copies that each carried every
    feature (about 50 on a tile's path; at most 26 now), most of them inside the sub-tile loop;
  * the copies are whole: every basic block that holds a piece of a tile end (LDS transposition or 16-byte store) holds all of it,
    the read-back of four sub-tiles = 16 ds_read_b128 (20 with the pooled tiles).  A block has no branch inside and no branch
    target but its first instruction, so no branch leads into or out of a sub-tile step; their number is 4 | 12;
  * every buffer_store_dwordx4 is followed by s_nop (og_buffer_store16's wait state);
  * registers: no scratch, 256 AGPRs, VGPRs within the budget of tests/test_isa_wino_loop.py (231 | 226).
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

COPIES = {2: 4, 1: 12}
HEAD_COPIES = {2: 0, 1: 8}
PK_ADD_TRANSFORM = 192
PK_ADD_MAX = {nt: PK_ADD_TRANSFORM + 24 * HEAD_COPIES[nt] for nt in (2, 1)}
MOV_MAX = {nt: 4 + 13 * HEAD_COPIES[nt] for nt in (2, 1)}
MUL_MAX = {2: 2 * 6 + 2 * 12, 1: (2 * 6 + 2 * 12) + (4 * 14 + 2 * 6) + (4 * 20 + 2 * 6)}
VGPR_MAX = {2: 231, 1: 226}


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_wino_tail")
    tu, asm = d / "wino.hip", d / "wino.s"
    hdr = os.path.join(ROOT, "openglottal_amd", "csrc", "og_kernels.hpp")
    tu.write_text(f'#include "{hdr}"\ntemplate __global__ void k_conv_wino<2>(ConvArgs);\ntemplate __global__ void k_conv_wino<1>(ConvArgs);\n')
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", str(tu), "-o", str(asm)],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    tool = os.path.join(ROOT, "tools", "isa_wino_tail.py")
    out = subprocess.run([sys.executable, tool, str(asm), "--json"], check=True, capture_output=True, text=True).stdout
    print(subprocess.run([sys.executable, tool, str(asm)], check=True, capture_output=True, text=True).stdout)
    return {int(r["kernel"][-2]): r for r in json.loads(out)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("nt", [2, 1])
def test_output_transform_runs_on_accumulator_pairs(rows, nt):
    r = rows[nt]
    brief = {k: v for k, v in r.items() if k != "copies"}
    assert r["v_accvgpr_read_b32"] == 256, brief
    assert r["outside_copies"]["v_pk_add_f32"] == PK_ADD_TRANSFORM and r["v_pk_add_f32"] <= PK_ADD_MAX[nt], brief
    assert r["v_mov_b32_from_vgpr"] == 0 and r["v_mov_b32"] <= MOV_MAX[nt], brief
    assert r["scratch"] == 0 and r["agprs"] <= 256 and r["vgprs"] <= VGPR_MAX[nt], brief


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("nt", [2, 1])
def test_tile_end_copies_are_whole_and_their_addresses_run_in_sgprs(rows, nt):
    r = rows[nt]
    brief = {k: v for k, v in r.items() if k != "copies"}
    assert len(r["copies"]) == COPIES[nt] and r["split_copies"] == 0, (brief, r["copies"])
    assert all(c["ds_read_b128"] in (16, 20) for c in r["copies"]), r["copies"]
    assert r["s_mul_i32"] <= MUL_MAX[nt], brief
    assert r["buffer_store_dwordx4"] > 0 and r["store16_without_nop"] == 0, brief
