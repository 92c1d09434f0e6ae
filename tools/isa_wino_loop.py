"""Static instruction audit of the chunk loop of k_conv_wino<1> and <2>: what one wave issues per chunk next to its 64 * NT
MFMAs (the kernel runs one wave per SIMD, so every instruction between two MFMAs takes issue time from the matrix pipe).
For each instantiation it finds the loop whose body holds 64 * NT MFMAs (the steady-state chunk, NXT = true) and the
straight-line copy behind it (the peeled last chunk), and prints one table row + the histogram of the MFMA gaps.
usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only openglottal_amd/csrc/og_api.hip -o /tmp/api.s
       python tools/isa_wino_loop.py /tmp/api.s [--json]"""
import collections, json, os, re, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_hazards import dma_operand_overwrites, operands   # noqa: E402  (the rule lives there, judged over every kernel)

BRANCH = ("s_cbranch", "s_branch")
M0_IMPLICIT = ("s_movrel", "v_movrel", "ds_gws", "v_interp", "s_sendmsg", "ds_add_gs", "ds_sub_gs", "ds_append", "ds_consume")


def kind(op):
    m = op.split()[0]
    if m.startswith("v_mfma") or m.startswith("v_smfma"):
        return "mfma"
    if (m.startswith("buffer_load") or m.startswith("global_load")) and re.search(r"\blds\b|_lds_", op):
        return "dma"
    if m.startswith("ds_read") or m.startswith("ds_load"):
        return "ds_read"
    if m.startswith("ds_write") or m.startswith("ds_store"):
        return "ds_write"
    if m == "v_pk_add_f32":
        return "v_pk_add"
    if m.startswith("v_"):
        return "valu"
    if m.startswith(BRANCH):
        return "branch"
    if m == "s_nop":
        return "s_nop"
    if m == "s_waitcnt":
        return "s_waitcnt"
    if m in ("s_barrier", "s_setprio", "s_sleep", "s_endpgm"):
        return "other"
    if m.startswith("s_load") or m.startswith("s_buffer_load") or m == "s_memtime" or m == "s_memrealtime":
        return "smem"
    if m.startswith("s_"):
        return "salu"
    return "other"


def reads_m0(op):
    m = op.split()[0]
    if m.startswith(M0_IMPLICIT) or " gds" in op:
        return True
    ops = operands(op)
    stores = m.startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_setreg"))   # no destination operand
    return any(re.fullmatch(r"m0", o) for o in (ops if stores else ops[1:]))


def writes_m0(op):
    m = op.split()[0]
    ops = operands(op)
    return bool(ops) and ops[0] == "m0" and m.startswith("s_") and not m.startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_setreg"))


def function(src, label):
    i = next(k for k, l in enumerate(src) if l.startswith(label + ":"))
    j = next(k for k, l in enumerate(src) if k > i and ".amdhsa_kernel" in l)
    e = next(k for k, l in enumerate(src) if k > j and "; ScratchSize" in l)
    ins, labels = [], {}
    for l in src[i + 1:j]:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        ins.append(t)
    meta = {}
    for l in src[j:e + 1]:
        for key, pat in (("scratch", r"\.amdhsa_private_segment_fixed_size (\d+)"), ("vgprs", r"; NumVgprs: (\d+)"), ("agprs", r"; NumAgprs: (\d+)")):
            m = re.search(pat, l)
            if m:
                meta[key] = int(m.group(1))
    return ins, labels, meta


def gaps_of(body):
    """instruction counts in front of the first MFMA, between consecutive MFMAs, and behind the last one"""
    g, n = [], 0
    for op in body:
        if kind(op) == "mfma":
            g.append(n); n = 0
        else:
            n += 1
    return g[0] if g else n, g[1:], n


def audit(src, nt):
    label = f"_Z11k_conv_winoILi{nt}EEv8ConvArgs"
    ins, labels, meta = function(src, label)
    want = 64 * nt
    # loops = backward branches; the chunk loop = header .. LAST back edge to that header, with `want` MFMAs in between
    loops = {}
    for k, op in enumerate(ins):
        if op.startswith(BRANCH):
            tgt = labels.get(op.split()[1])
            if tgt is not None and tgt <= k:
                loops[tgt] = max(loops.get(tgt, -1), k)
    cand = [(h, e) for h, e in loops.items() if sum(kind(o) == "mfma" for o in ins[h:e + 1]) == want]
    r = {"kernel": f"k_conv_wino<{nt}>", "loop_found": len(cand) == 1, "dma_operand_overwritten_next": dma_operand_overwrites(ins), **meta}
    if len(cand) != 1:
        return r
    h, e = cand[0]
    body = ins[h:e + 1]
    cnt = collections.Counter(kind(o) for o in body)
    head, gaps, tail = gaps_of(body)
    inside = {l for l, p in labels.items() if h < p <= e}
    r.update({
        "body": {k: cnt.get(k, 0) for k in ("mfma", "ds_read", "ds_write", "dma", "v_pk_add", "valu", "salu", "s_nop", "branch", "s_waitcnt", "smem", "other")},
        "total": len(body),
        "valu_ops": sorted(collections.Counter(o.split()[0] for o in body if kind(o) == "valu").items()),
        "guard_branches": sum(1 for o in body if o.startswith(BRANCH) and o.split()[1] in inside),
        "m0_reads": sum(reads_m0(o) for o in body), "m0_writes": sum(writes_m0(o) for o in body),
        "gap_max": max(gaps) if gaps else 0, "gap_head": head, "gap_tail": tail,
        "gap_hist": sorted(collections.Counter(gaps).items()),
    })
    # the peeled last chunk: everything behind the loop up to the last MFMA of the kernel
    rest = ins[e + 1:]
    idx = [k for k, o in enumerate(rest) if kind(o) == "mfma"]
    peel = rest[:idx[-1] + 1] if idx else []
    second = rest[idx[want // 2 - 1] + 1:idx[-1] + 1] if len(idx) >= want // 2 else []
    pc = collections.Counter(kind(o) for o in peel)
    r["peel"] = {"mfma": pc.get("mfma", 0), "dma": pc.get("dma", 0), "dma_second_group": sum(kind(o) == "dma" for o in second),
                 "v_pk_add": pc.get("v_pk_add", 0), "valu": pc.get("valu", 0), "ds_write": pc.get("ds_write", 0), "branch": pc.get("branch", 0),
                 "total": len(peel)}
    r["mfma_before_loop"] = sum(kind(o) == "mfma" for o in ins[:h])
    return r


def main():
    src = open(sys.argv[1]).read().split("\n")
    rows = [audit(src, nt) for nt in (2, 1)]
    if "--json" in sys.argv:
        print(json.dumps(rows))
        return
    cols = ("mfma", "ds_read", "ds_write", "dma", "v_pk_add", "valu", "salu", "s_nop", "branch", "s_waitcnt", "smem", "other")
    print(f"{'steady-state chunk':20s} " + " ".join(f"{c:>9s}" for c in cols) + f" {'total':>6s}")
    for r in rows:
        if not r["loop_found"]:
            print(f"{r['kernel']:20s} no loop with {64 * int(r['kernel'][-2])} MFMAs found")
            continue
        print(f"{r['kernel']:20s} " + " ".join(f"{r['body'][c]:9d}" for c in cols) + f" {r['total']:6d}")
    for r in rows:
        if not r["loop_found"]:
            continue
        print(f"{r['kernel']}: VGPRs {r['vgprs']} AGPRs {r['agprs']} scratch {r['scratch']}; LDS-DMAs of the kernel with an operand register written by the next "
              f"instruction {r['dma_operand_overwritten_next']}; branches into the body (guards) {r['guard_branches']}; "
              f"M0 reads {r['m0_reads']} writes {r['m0_writes']}; other VALU {r['valu_ops']}")
        print(f"  MFMA gaps (instructions between two MFMAs: count): {r['gap_hist']}; largest {r['gap_max']}, before the first MFMA {r['gap_head']}, "
              f"behind the last {r['gap_tail']}")
        p = r["peel"]
        print(f"  last chunk (peeled): {p['mfma']} MFMA, {p['dma']} LDS-DMA ({p['dma_second_group']} in its second group), {p['v_pk_add']} v_pk_add, "
              f"{p['valu']} other VALU, {p['ds_write']} ds_write, {p['branch']} branches, {p['total']} instructions")


if __name__ == "__main__":
    main()
