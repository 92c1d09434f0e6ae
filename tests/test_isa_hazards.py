"""Wait states that hipcc leaves unpadded around inline asm, audited on the listing (no GPU needed: hipcc cross-compiles).

hipcc's hazard recognizer does not look inside an asm statement.  One wave-dependent dropped store came from there (DESIGN.md,
"Finding": `v_readlane_b32 s40..s43` directly in front of og_buffer_store16's block in k_conv_mfma_p<1, 0, 16, 9>), the scan that
found it was never kept, and every change of register allocation moves these sequences.  tools/isa_hazards.py walks the control
flow graph of every kernel of the listing and judges

  R1  VALU write of an SGPR / VCC -> asm buffer_* / global_* reading it: 5 wait states,
  R2  SALU write of M0 -> LDS-DMA: 1 wait state,
  R3  12 / 16-byte store (asm or not) -> VALU write of its data VGPRs: 2 wait states (also counted below 1),
  R4  LDS-DMA -> the next instruction writes one of its operand registers,

in a closed world: an asm mnemonic it cannot classify, an asm VMEM whose operands it cannot read, or a site with a call / return
inside its window is a failure, not a skip.  The counts come from the GFX9 hazard table as og_kernels.hpp cites it (5; 1) and from
"an asm store of 3 or 4 dwords ends with s_nop 1" (2) -- not from what the shipped code happens to have.

Three layers:
  * synthetic listings of a few lines, a violating and a clean case per rule -- the violating ones fail if the rule is switched
    off, the clean ones if it over-reports.  They need no compiler;
  * the shipped listing: zero violations of every rule, nothing unclassified, every asm VMEM instruction judged (the tool's count
    against a plain count of such lines);
  * three mutants of the shipped listing (text edits in memory) that undo a pad the sources carry: the audit must find exactly the
    stores of DESIGN's finding (10 in k_conv_mfma_p<1, 0, 16, 9> + 6 in <1, 0, 16, 3>, no other kernel), every LDS-DMA block whose
    M0 wait state was removed, and at least the 46 stores whose data registers the next instruction writes.
"""
import collections
import json
import os
import re
import subprocess
import sys

import pytest

import isa_listing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_hazards as H   # noqa: E402

needs_hipcc = pytest.mark.skipif(not isa_listing.available(), reason="hipcc not available")

STORE = "buffer_store_dwordx4 v[10:13], v4, s[40:43], s2 offen"
DMA = "buffer_load_dwordx4 v1, s[4:7], s2 offen lds"


def listing(body, name="_Z1kv", kernel=True):
    """a hipcc -S listing of one function; `{` and `}` on lines of their own open and close an asm block"""
    out = [f"{name}:"]
    for l in body.strip("\n").split("\n"):
        l = l.strip()
        out.append({"{": "\t;;#ASMSTART", "}": "\t;;#ASMEND"}.get(l, l if l.endswith(":") else "\t" + l))
    out += ["\ts_endpgm", ".Lfunc_end0:"] + ([f"\t.amdhsa_kernel {name}", "\t.end_amdhsa_kernel"] if kernel else [])
    return out


def audit(body, **kw):
    rep = H.audit(listing(body, **kw))
    assert not rep["unclassified"] and not rep["unparsed"], rep
    return rep


def clean(rep):
    R = rep["rules"]
    return not (R["R1"]["violations"] or R["R2"]["violations"] or R["R3"]["below_2"] or R["R4"]["violations"] or rep["undecided"])


# ---- R1: VALU writes an SGPR, an asm VMEM reads it: 5 states ----------------------------------------------------------------
@pytest.mark.parametrize("pad, found", [("", 0), ("s_nop 3", 4), ("s_nop 4", None), ("s_nop 0\ns_nop 2", 4), ("s_mov_b32 s9, 0\ns_nop 3", None)])
def test_r1_writer_in_front_of_the_block(pad, found):
    rep = audit(f"v_readlane_b32 s41, v9, 3\n{{\n{pad}\n{STORE}\ns_nop 1\n}}".replace("\n\n", "\n"))
    v = rep["rules"]["R1"]["violations"]
    if found is None:
        assert clean(rep) and rep["rules"]["R1"]["slack"] == {"0": 1}, rep
    else:
        assert [(s["states"], s["at"], s["other"]) for s in v] == [(found, STORE, "v_readlane_b32 s41, v9, 3")], rep


@pytest.mark.parametrize("writer, hit", [
    ("v_readfirstlane_b32 s2, v0", True),                     # the soffset
    ("v_cmp_gt_i32_e64 s[42:43], v0, v1", True),              # v_cmp with an SGPR pair as destination
    ("v_add_co_u32_e64 v5, s[2:3], v1, v2", True),            # carry-out
    ("v_div_scale_f32 v5, s[40:41], v1, v1, v2", True),
    ("v_readlane_b32 s44, v9, 3", False),                     # another SGPR
    ("v_cmp_gt_i32_e32 vcc, v0, v1", False),                  # VCC is no operand of this store
    ("v_add_u32_e32 v5, s2, v1", False),                      # reads s2
    ("s_mov_b32 s2, s9", False),                              # a scalar-ALU write needs no wait state
])
def test_r1_which_writers_count(writer, hit):
    rep = audit(f"{writer}\n{{\n{STORE}\ns_nop 1\n}}")
    assert len(rep["rules"]["R1"]["violations"]) == int(hit), rep


def test_r1_saddr_of_a_global_transfer_and_compiler_vmem_left_to_the_compiler():
    rep = audit("v_readfirstlane_b32 s8, v0\n{\ns_mov_b32 m0, s3\ns_nop 0\nglobal_load_lds_dwordx4 v1, s[8:9]\n}")
    assert [s["states"] for s in rep["rules"]["R1"]["violations"]] == [2], rep
    rep = audit(f"v_readlane_b32 s41, v9, 3\n{STORE}\ns_nop 1")          # not in an asm block: hipcc's recognizer owns it
    assert clean(rep) and rep["rules"]["R1"]["judged"] == 0, rep


JOIN = """
s_cbranch_scc1 .LBB0_2
v_readlane_b32 s40, v9, 0
%s
s_branch .LBB0_3
.LBB0_2:
s_mov_b32 s40, 0
s_nop 7
.LBB0_3:
{
%s
s_nop 1
}
"""


def test_r1_writer_on_the_branch_source_path_of_a_join():
    """the fall-through path into the block is long and clean; the writer sits on the path that BRANCHES to the join"""
    rep = audit(JOIN % ("s_nop 1", STORE))
    assert [(s["states"], s["other"]) for s in rep["rules"]["R1"]["violations"]] == [(3, "v_readlane_b32 s40, v9, 0")], rep   # s_nop 1 + s_branch
    assert clean(audit(JOIN % ("s_nop 3", STORE)))                                                                              # 4 + s_branch


LOOP = """
s_mov_b32 s2, 0
.LBB0_1:
{
%s
s_nop 1
}
s_add_i32 s2, s2, 16
s_cmp_lt_u32 s2, s20
v_readlane_b32 s43, v9, 3
%s
s_cbranch_scc1 .LBB0_1
"""


def test_r1_writer_reaches_the_block_around_a_loop_back_edge():
    rep = audit(LOOP % (STORE, "s_nop 2"))
    assert [(s["states"], s["other"]) for s in rep["rules"]["R1"]["violations"]] == [(4, "v_readlane_b32 s43, v9, 3")], rep     # s_nop 2 + the branch
    assert clean(audit(LOOP % (STORE, "s_nop 3")))
    assert clean(audit(LOOP % ("s_nop 4\n" + STORE, "")))            # the pad inside the string, as og_buffer_store16 carries it


# ---- R2: SALU writes M0, LDS-DMA: 1 state -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dma", [DMA, "global_load_lds_dwordx4 v[0:1], off"])
def test_r2_m0_write_and_transfer(dma):
    rep = audit(f"{{\ns_mov_b32 s9, m0\ns_mov_b32 m0, s3\n{dma}\ns_mov_b32 m0, s9\n}}")
    assert [(s["states"], s["other"]) for s in rep["rules"]["R2"]["violations"]] == [(0, "s_mov_b32 m0, s3")], rep
    rep = audit(f"{{\ns_mov_b32 s9, m0\ns_mov_b32 m0, s3\ns_nop 0\n{dma}\ns_mov_b32 m0, s9\n}}")
    assert clean(rep) and rep["rules"]["R2"]["slack"] == {"0": 1} and rep["rules"]["R4"]["m0_written_next"] == 1, rep


def test_r2_m0_written_by_the_compiler_in_front_of_the_block():
    assert len(audit(f"s_add_i32 m0, s3, 0x400\n{{\n{DMA}\n}}")["rules"]["R2"]["violations"]) == 1
    assert clean(audit(f"s_add_i32 m0, s3, 0x400\n{{\ns_nop 0\n{DMA}\n}}"))
    assert clean(audit(f"s_mov_b32 m0, s3\n{{\ns_and_saveexec_b64 s[10:11], s[12:13]\n{DMA}\ns_mov_b64 exec, s[10:11]\n}}"))
    assert clean(audit(f"s_mov_b32 s9, m0\n{{\n{DMA}\n}}"))          # reads M0
    # the block at a loop head: M0 written in front of the loop without a pad (first trip) | on the back edge (the branch is the state)
    loop = f".LBB0_1:\n{{\n{DMA}\n}}\ns_cmp_lt_u32 s2, s20\ns_add_i32 m0, m0, 64\ns_cbranch_scc1 .LBB0_1"
    rep = audit("s_mov_b32 m0, s3\n" + loop)
    assert [(s["states"], s["other"]) for s in rep["rules"]["R2"]["violations"]] == [(0, "s_mov_b32 m0, s3")], rep
    rep = audit("s_mov_b32 m0, s3\ns_nop 0\n" + loop)
    assert clean(rep) and rep["rules"]["R2"]["slack"] == {"0": 1}, rep


# ---- R3: 12 / 16-byte store, VALU write of its data VGPRs: 2 states ---------------------------------------------------------
@pytest.mark.parametrize("store", [STORE, "global_store_dwordx4 v[0:1], v[10:13], off sc1", "buffer_store_dwordx3 v[10:12], off, s[40:43], 0 offset:16"])
@pytest.mark.parametrize("pad, below_1, below_2", [("", 1, 1), ("s_nop 0", 0, 1), ("s_nop 1", 0, 0), ("s_add_i32 s9, s9, 1", 0, 1)])
def test_r3_distance_of_the_writer(store, pad, below_1, below_2):
    rep = audit(f"{{\n{store}\n{pad}\n}}\nv_pk_fma_f32 v[12:13], v[0:1], v[46:47], v[44:45]".replace("\n\n", "\n"))
    R3 = rep["rules"]["R3"]
    assert (len(R3["below_1"]), len(R3["below_2"])) == (below_1, below_2), rep
    rep = audit(f"{store}\n{pad}\nv_pk_fma_f32 v[12:13], v[0:1], v[46:47], v[44:45]".replace("\n\n", "\n"))       # hipcc's own store
    assert (len(rep["rules"]["R3"]["below_1"]), len(rep["rules"]["R3"]["below_2"])) == (below_1, below_2), rep


@pytest.mark.parametrize("nxt", ["v_cmp_gt_f32_e32 vcc, v10, v11", "v_cmp_gt_f32_e64 s[10:11], v10, v11", "v_pk_fma_f32 v[14:15], v[10:11], v[12:13], v[10:11]",
                                 "v_readlane_b32 s10, v10, 0", "ds_read_b128 v[10:13], v1", "s_mov_b32 s10, 0"])
def test_r3_what_is_no_valu_write_of_the_data(nxt):
    assert clean(audit(f"{{\n{STORE}\n}}\n{nxt}\ns_nop 1"))


def test_r3_narrow_stores_are_not_judged_and_wide_writers_are():
    assert audit("buffer_store_dwordx2 v[10:11], v4, s[40:43], s2 offen\nv_mov_b32_e32 v10, 0")["rules"]["R3"]["judged"] == 0
    for w in ("v_mov_b32_e32 v13, 0", "v_ldexp_f32 v10, v1, v2", "v_cndmask_b32_e32 v11, v1, v2, vcc", "v_swap_b32 v99, v12",
              "v_mfma_f32_32x32x2_f32 v[0:15], v1, v2, v[0:15]", "v_accvgpr_read_b32 v12, a3"):
        assert len(audit(f"{{\n{STORE}\n}}\n{w}")["rules"]["R3"]["below_1"]) == 1, w


def test_r3_writer_at_a_branch_target_behind_the_store():
    body = "{\n%s\n%s\n}\ns_cbranch_scc1 .LBB0_2\ns_nop 7\ns_branch .LBB0_3\n.LBB0_2:\nv_mov_b32_e32 v11, 0\n.LBB0_3:\ns_nop 0"
    R3 = audit(body % (STORE, "s_nop 0"))["rules"]["R3"]              # s_nop 0 + the branch = 2 states
    assert not R3["below_2"] and R3["slack"] == {"0": 1}, R3
    R3 = audit((body % (STORE, "")).replace("\n\n", "\n"))["rules"]["R3"]
    assert [s["states"] for s in R3["below_2"]] == [1] and not R3["below_1"], R3


# ---- R4, the closed world, the command line ---------------------------------------------------------------------------------
@pytest.mark.parametrize("nxt, hit", [("v_add_u32_e32 v1, 16, v1", 1), ("s_add_i32 s2, s2, 64", 1), ("s_mov_b32 s5, 0", 1), ("v_add_u32_e32 v2, 16, v1", 0),
                                      ("s_mov_b32 m0, s9", 0), ("s_cmp_lt_u32 s2, s20", 0)])
def test_r4_operand_of_a_transfer_written_by_the_next_instruction(nxt, hit):
    rep = audit(f"s_mov_b32 m0, s3\n{{\ns_nop 0\n{DMA}\n}}\n{nxt}")
    assert len(rep["rules"]["R4"]["violations"]) == hit and H.dma_operand_overwrites([DMA, nxt]) == hit, rep
    assert rep["rules"]["R4"]["m0_written_next"] == int(nxt.startswith("s_mov_b32 m0")), rep


@pytest.mark.parametrize("line, key", [
    ("s_getreg_b32 s9, hwreg(HW_REG_MODE)", "unclassified"),                  # scalar, but no plain ALU prefix of the table
    ("s_memtime s[10:11]", "unclassified"),
    ("image_load v[0:3], v4, s[8:15]", "unclassified"),
    ("buffer_load_dwordx4 v1, ttmp[4:7], s2 offen lds", "unparsed"),
    ("buffer_store_dwordx4 v[10:13], v4, s[40:43], exec_lo offen", "unparsed"),
])
def test_closed_world_reports_what_it_cannot_classify_or_read(line, key):
    rep = H.audit(listing(f"{{\n{line}\n}}"))
    assert [s["at"] for s in rep[key]] == [line] and H.failed(rep), rep
    rep = H.audit(listing(line))            # outside an asm block it is hipcc's business -- but for a wide store, which R3 judges anywhere
    assert not rep["unclassified"] and H.failed(rep) == bool(H.store_width(line)), rep


def test_scalar_class_is_a_list_of_alu_prefixes():
    """a bare `s_` would classify every scalar instruction, whatever it does, as plain ALU"""
    assert all(len(p) > 3 and p.startswith(("s_", "v_", "ds_", "buffer_", "global_")) or p == "v_" for _, ps in H.ASM_CLASSES for p in ps)
    assert H.asm_class("s_mov_b32 m0, s3") == "salu" and H.asm_class("s_and_saveexec_b64 s[0:1], s[2:3]") == "salu"
    assert H.asm_class("s_frobnicate_b32 s0, s1") is None and H.asm_class("v_pk_add_f32 v[0:1], v[2:3], v[4:5]") == "valu"


def test_call_or_return_inside_a_window_is_not_judged_and_fails():
    rep = H.audit(listing(f"v_readlane_b32 s41, v9, 3\ns_swappc_b64 s[30:31], s[16:17]\n{{\n{STORE}\ns_nop 1\n}}"))
    assert [s["rule"] for s in rep["undecided"]] == ["R1"] and H.failed(rep), rep
    rep = H.audit(listing(f"s_swappc_b64 s[30:31], s[16:17]\n{{\ns_nop 4\n{STORE}\ns_nop 1\n}}"))       # 5 states: whatever came before is far enough
    assert not rep["undecided"] and not H.failed(rep), rep
    # the entry of a kernel is a clean start; the entry of a device function is its caller's last instruction
    assert not H.audit(listing(f"{{\n{STORE}\ns_nop 1\n}}"))["undecided"]
    assert len(H.audit(listing(f"{{\n{STORE}\ns_nop 1\n}}", kernel=False))["undecided"]) == 1


def test_command_line_exit_code_report_and_json(tmp_path):
    tool = os.path.join(ROOT, "tools", "isa_hazards.py")
    bad, good = tmp_path / "bad.s", tmp_path / "good.s"
    bad.write_text("\n".join(listing(f"v_readlane_b32 s41, v9, 3\n{{\n{STORE}\n}}\nv_mov_b32_e32 v10, 0")))
    good.write_text("\n".join(listing(f"v_readlane_b32 s41, v9, 3\n{{\ns_nop 4\n{STORE}\ns_nop 1\n}}\nv_mov_b32_e32 v10, 0")))
    p = subprocess.run([sys.executable, tool, str(bad), "--json"], capture_output=True, text=True)
    rep = json.loads(p.stdout)
    assert p.returncode == 1 and len(rep["rules"]["R1"]["violations"]) == 1 and len(rep["rules"]["R3"]["below_1"]) == 1, p.stdout
    p = subprocess.run([sys.executable, tool, str(good)], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = [l.split()[0] for l in p.stdout.splitlines() if re.match(r"R\d ", l)]
    assert rows == ["R1", "R2", "R3", "R3", "R4"], p.stdout          # one row per rule (R3 at 1 and at 2 states)
    assert "R1 (need 5): 0: 1" in p.stdout and "R3 (need 2): 0: 1" in p.stdout, p.stdout


# ---- the shipped listing ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shipped():
    src = isa_listing.lines()
    rep = H.audit(src)
    print(H.report(rep))
    return src, rep


def asm_lines(src):
    """(line index, stripped text) of every line inside an asm block -- a plain scan that shares nothing with the tool"""
    inside = False
    for k, l in enumerate(src):
        s = l.strip()
        if s.startswith(";;#ASMSTART"):
            inside = True
        elif s.startswith(";;#ASMEND"):
            inside = False
        elif inside and s:
            yield k, s


def short(kernel):
    m = re.match(r"_Z\d+(k_\w+?)I((?:L[ib]\d+E)+)E", kernel)
    return m.group(1) + "<" + ",".join(re.findall(r"L[ib](\d+)E", m.group(2))) + ">" if m else kernel


def per_kernel(sites):
    return dict(collections.Counter(short(s["kernel"]) for s in sites))


@needs_hipcc
def test_shipped_listing_has_no_unpadded_hazard_and_nothing_unjudged(shipped):
    src, rep = shipped
    R = rep["rules"]
    assert not rep["unclassified"], rep["unclassified"][:5]
    assert not rep["unparsed"], rep["unparsed"][:5]
    assert not rep["undecided"], rep["undecided"][:5]
    vmem = sum(1 for _, s in asm_lines(src) if re.match(r"(buffer|global|flat|scratch|tbuffer)_", s))
    print("VMEM instructions inside asm blocks:", vmem)
    assert vmem > 0 and rep["asm_vmem_judged"] == vmem == R["R1"]["judged"] == sum(rep["asm_vmem"].values()), (vmem, rep["asm_vmem_judged"], rep["asm_vmem"])
    dma = sum(1 for l in src if re.match(r"\s+(buffer_load\w+ .*\blds\b|global_load_lds_)", l))
    assert dma > 0 and R["R2"]["judged"] == dma == R["R4"]["judged"], (dma, R["R2"]["judged"], R["R4"]["judged"])
    wide = sum(1 for l in src if re.match(r"\s+(buffer|global|flat)_store_dwordx[34]\b", l))
    assert wide > 0 and R["R3"]["judged"] == wide, (wide, R["R3"]["judged"])
    assert rep["kernels"] >= 100, rep["kernels"]
    assert not R["R1"]["violations"], per_kernel(R["R1"]["violations"])
    assert not R["R2"]["violations"], per_kernel(R["R2"]["violations"])
    assert not R["R4"]["violations"], per_kernel(R["R4"]["violations"])
    assert not R["R3"]["below_1"], per_kernel(R["R3"]["below_1"])
    assert not R["R3"]["below_2"], per_kernel(R["R3"]["below_2"])          # two states behind every 12 / 16-byte store
    assert not H.failed(rep)
    assert all(int(k) >= 0 for r in ("R1", "R2", "R3") for k in R[r]["slack"] if k.lstrip("-").isdigit()), R


def mutate(src, pick):
    """a copy of the listing with the asm-block lines dropped / replaced that pick(prev, line, next) -> None | '' | text names"""
    body = list(asm_lines(src))
    out, n = list(src), 0
    for (_, a), (k, s), (_, b) in zip([(0, "")] + body, body, body[1:] + [(0, "")]):
        new = pick(a, s, b)
        if new is not None:
            out[k] = ("\t" + new) if new else ""
            n += 1
    return out, n


@needs_hipcc
def test_mutant_without_the_pad_in_front_of_the_store_is_the_historic_bug(shipped):
    """every `s_nop 4` that opens a store block becomes `s_nop 0`: what shipped before DESIGN's finding"""
    src, _ = shipped
    mut, n = mutate(src, lambda a, s, b: "s_nop 0" if s == "s_nop 4" and re.match(r"(buffer|global)_store_", b) else None)
    assert n > 0
    v = H.audit(mut)["rules"]["R1"]["violations"]
    assert per_kernel(v) == {"k_conv_mfma_p<1,0,16,9>": 10, "k_conv_mfma_p<1,0,16,3>": 6}, per_kernel(v)
    assert all(s["other"].startswith("v_readlane_b32") and s["at"].startswith("buffer_store_dwordx4") for s in v), v
    assert len({s["line"] for s in v}) == 16


@needs_hipcc
def test_mutant_without_the_m0_wait_state_is_flagged_at_every_block(shipped):
    """the `s_nop 0` between an in-string write of M0 and its transfer is removed"""
    src, _ = shipped
    is_dma = lambda s: bool(re.match(r"buffer_load\w+ .*\blds\b|global_load_lds_", s))
    mut, n = mutate(src, lambda a, s, b: "" if s == "s_nop 0" and re.match(r"s_\w+ m0,", a) and is_dma(b) else None)
    assert n > 0
    v = H.audit(mut)["rules"]["R2"]["violations"]
    print("LDS-DMA blocks with their own M0 write:", n)
    assert len(v) == n == len({s["line"] for s in v}), (len(v), n)
    assert all(s["states"] == 0 and s["other"].split()[1] == "m0," for s in v)


R3_TODAY = {   # stores whose data registers the instruction directly behind the block's trailing nop writes, per kernel
    "k_conv_wino<1>": 5, "k_conv_wino<2>": 1,
    "k_conv_mfma_o<2,0,16,2,0,0>": 10, "k_conv_mfma_o<2,0,8,3,0,1>": 3, "k_conv_mfma_o<2,0,8,3,0,0>": 3, "k_conv_mfma_o<2,0,8,4,0,0>": 3,
    "k_conv_mfma_h<2,0,16,2,0,0>": 5, "k_conv_mfma_h<2,0,8,3,0,0>": 2,
    "k_conv_mfma_f<2,0,16,2,0,0>": 3, "k_conv_mfma_f<2,0,16,2,0,1>": 2, "k_conv_mfma_f<1,0,16,2,0,0>": 1, "k_conv_mfma_f<2,0,8,3,0,0>": 1,
    "k_conv_mfma_f<2,1,8,3,0,0>": 1,
    "k_conv_mfma_fy<2,3,3,0>": 2, "k_conv_mfma_fy<2,0,3,0>": 2, "k_conv_mfma_fy<2,2,3,0>": 2,
}


@needs_hipcc
def test_mutant_without_the_pad_behind_the_store_shows_the_overwritten_data_registers(shipped):
    """the `s_nop` behind every asm store is removed: hipcc's next instruction stands directly behind the store"""
    src, _ = shipped
    mut, n = mutate(src, lambda a, s, b: "" if s.startswith("s_nop") and re.match(r"(buffer|global)_store_dwordx[34]\b", a) else None)
    stores = sum(1 for _, s in asm_lines(src) if re.match(r"(buffer|global)_store_dwordx[34]\b", s))
    assert n == stores > 0, (n, stores)
    v = H.audit(mut)["rules"]["R3"]["below_1"]
    got = per_kernel(v)
    print("stores with a data register written by the next instruction:", len(v), got)
    assert sum(R3_TODAY.values()) == 46 and len(v) >= 46, len(v)
    assert all(got.get(k, 0) >= c for k, c in R3_TODAY.items()), {k: (got.get(k, 0), c) for k, c in R3_TODAY.items() if got.get(k, 0) < c}
    assert all(s["states"] == 0 for s in v)
