"""tools/isa_diff.py on short synthetic listings (no compiler, no GPU): what it must call equal and what it must not.

The tool is the yardstick of source refactors of the kernels (profiles/r10_isa_diff.txt): a pair it wrongly calls equal hides a
lost register or an added LDS read, a pair it wrongly calls different makes every refactor look like a change.
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_diff as D   # noqa: E402

BODY = """
s_load_dwordx4 s[4:7], s[0:1], 0x0
v_lshlrev_b32_e32 v1, 4, v0
s_waitcnt lgkmcnt(0)
buffer_load_dwordx4 v[2:5], v1, s[4:7], 0 offen
s_cmp_lt_i32 s8, 1
s_cbranch_scc1 .LBB0_2
.LBB0_1:
ds_read_b128 v[6:9], v1
s_waitcnt lgkmcnt(0)
v_mfma_f32_32x32x2_f32 a[0:15], v6, v2, a[0:15]
v_mfma_f32_32x32x2_f32 a[0:15], v7, v3, a[0:15]
s_add_i32 s8, s8, -1
s_cmp_lg_u32 s8, 0
s_cbranch_scc1 .LBB0_1
.LBB0_2:
s_barrier
global_store_dwordx4 v[10:11], v[2:5], off
"""


def listing(body, name="_Z1kv", vgprs=12, lds=4096):
    out = [f"{name}:"] + [l if l.endswith(":") else "\t" + l for l in body.strip("\n").split("\n")]
    out += ["\ts_endpgm", ".Lfunc_end0:", f"\t.amdhsa_kernel {name}", "\t.end_amdhsa_kernel", "; Kernel info:", "; TotalNumSgprs: 16",
            f"; NumVgprs: {vgprs}", "; NumAgprs: 16", "; ScratchSize: 0", f"; LDSByteSize: {lds} bytes/workgroup (compile time only)", "; Occupancy: 8"]
    return out


def classes(a, b):
    rows, exceptions = D.compare(D.symbols(a), D.symbols(b))
    return {name: cls for name, cls, _ in rows}, rows, exceptions


def test_identical_pair():
    c, _, exceptions = classes(listing(BODY), listing(BODY))
    assert c == {"_Z1kv": "identical"} and not exceptions


def test_register_renamed_pair():
    other = BODY.replace("v[6:9]", "v[16:19]").replace("v6,", "v16,").replace("v7,", "v17,").replace("s8", "s12").replace(".LBB0_", ".LBB3_")
    assert other != BODY
    c, _, exceptions = classes(listing(BODY), listing(other))
    assert c == {"_Z1kv": "renamed"} and not exceptions


def test_set_up_difference_outside_the_mfma_blocks():
    other = BODY.replace("v_lshlrev_b32_e32 v1, 4, v0", "v_mul_u32_u24_e32 v1, 16, v0")
    c, rows, exceptions = classes(listing(BODY), listing(other))
    assert c == {"_Z1kv": "set-up"} and not exceptions, rows


def test_added_ds_read_is_a_hard_failure():
    other = BODY.replace("s_waitcnt lgkmcnt(0)\nv_mfma", "ds_read_b128 v[20:23], v1 offset:16\ns_waitcnt lgkmcnt(0)\nv_mfma")
    assert other.count("ds_read_b128") == 2
    c, rows, _ = classes(listing(BODY), listing(other))
    assert c == {"_Z1kv": "HARD"}
    assert "+ds_read_b128" in rows[0][2], rows


def test_compiler_nop_is_not_part_of_the_sequence_but_breaks_the_mfma_block():
    other = BODY.replace("s_add_i32 s8, s8, -1", "s_nop 1\ns_add_i32 s8, s8, -1")
    c, _, exceptions = classes(listing(BODY), listing(other))
    assert c == {"_Z1kv": "MFMA-BLOCK"}
    assert len(exceptions) == 1 and "+s_nop 1" in exceptions[0][2]


def test_changed_vgpr_count_is_a_hard_failure():
    c, rows, _ = classes(listing(BODY), listing(BODY, vgprs=13))
    assert c == {"_Z1kv": "HARD"}
    assert "NumVgprs 12 -> 13" in rows[0][2], rows
    c, rows, _ = classes(listing(BODY), listing(BODY, lds=8192))
    assert c == {"_Z1kv": "HARD"} and "LDS 4096 -> 8192" in rows[0][2], rows


def test_missing_symbol_is_a_hard_failure():
    c, _, _ = classes(listing(BODY) + listing(BODY, name="_Z2k2v"), listing(BODY))
    assert c == {"_Z1kv": "identical", "_Z2k2v": "HARD"}


def test_command_line_exit_codes(tmp_path):
    a, b, h = tmp_path / "a.s", tmp_path / "b.s", tmp_path / "h.s"
    a.write_text("\n".join(listing(BODY)))
    b.write_text("\n".join(listing(BODY.replace("v6,", "v16,"))))
    h.write_text("\n".join(listing(BODY, vgprs=13)))
    tool = os.path.join(ROOT, "tools", "isa_diff.py")
    ok = subprocess.run([sys.executable, tool, str(a), str(b)], capture_output=True, text=True)
    assert ok.returncode == 0 and "1 symbols: 0 identical, 1 renamed" in ok.stdout and "asm VMEM sites judged 0 -> 0" in ok.stdout, ok.stdout + ok.stderr
    bad = subprocess.run([sys.executable, tool, str(a), str(h)], capture_output=True, text=True)
    assert bad.returncode == 1 and "HARD" in bad.stdout, bad.stdout + bad.stderr
