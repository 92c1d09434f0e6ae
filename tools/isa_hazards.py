"""CFG-aware wait-state audit of a hipcc -S listing: the hazards hipcc leaves unpadded around inline asm, over EVERY kernel.

hipcc's hazard recognizer treats an asm statement as one opaque instruction: it neither sees a consumer inside the string nor
pads a producer in front of it.  One dropped store came from there ("Finding": v_readlane_b32 s40..s43 directly in
front of og_buffer_store16's block), and every change of register allocation moves these sequences.  This tool reads the listing
the way the hardware runs it -- a backward / forward walk over all predecessors / successors of a site (fall-through, branch
sources, loop back edges), one wait state per instruction and N + 1 for `s_nop N` -- and judges four rules:

  R1  VALU writes an SGPR / VCC (v_readlane, v_readfirstlane, v_cmp* with a scalar destination, the carry-out of *_co_*,
      v_div_scale, v_mad_u64_u32), an ASM buffer_* / global_* reads it as descriptor, soffset or saddr: 5 wait states.
      [GFX9 "VALU writes SGPR -> VMEM reads that SGPR"; og_kernels.hpp, og_buffer_store16: the `s_nop 4` that opens the string]
  R2  SALU writes M0, an LDS-DMA (buffer_load ... lds, global_load_lds_*) uses it: 1 wait state.
      [og_kernels.hpp, glds16 / glds16b / glds16b_m0: "the wait state between an M0 write and its LDS-DMA use"]
  R3  a buffer_ / global_ / flat_store of 3 or 4 dwords, in asm or not, then a VALU write of its data VGPRs: reported below 1
      state (the GFX9 rule, tools/isa_store_hazard.py's "very next instruction") and below 2 (what the gfx940 family asks for:
      an asm store "ends with s_nop 1").  [og_kernels.hpp, og_buffer_store16 / og_store16_dev]
  R4  an LDS-DMA whose operand registers (VGPR offset, descriptor, soffset) are written by the next instruction.
      [og_kernels.hpp, glds16b_m0<PAD>]  A write of M0 there is counted apart and is no violation: it is the restore that
      glds16 / glds16b place behind their transfer on purpose.

Closed world: every mnemonic inside an asm block must fall into a class of ASM_CLASSES by prefix (the scalar class is a list of
ALU prefixes, not `s_`: anything scalar that is not plain ALU stays unclassified), every asm VMEM must parse into the operand
shape of its form, and no site may have a call or a return (s_swappc / s_setpc: the walk cannot follow them) inside its window.
What does not is reported, never skipped, and fails the test.

For every rule the report gives the histogram of slack (wait states present - needed) at the sites where a producer lies
within HORIZON states; "far" = none that near on any path.

usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only openglottal_amd/csrc/og_api.hip -o /tmp/api.s
       python tools/isa_hazards.py /tmp/api.s [--json]       exit code 1 on any violation / unclassified / unparsed"""
import collections, json, re, sys

HORIZON = 8          # states beyond a rule's need up to which the nearest producer is still looked for (the slack histogram)
NEED = {"R1": 5, "R2": 1, "R3": 2}

# mnemonic classes of the inside of asm blocks, by prefix, first match wins
SALU_PREFIXES = ("s_mov", "s_cmov", "s_not", "s_and", "s_andn2", "s_or", "s_orn2", "s_xor", "s_nand", "s_nor", "s_xnor", "s_add", "s_sub",
                 "s_mul", "s_lshl", "s_lshr", "s_ashr", "s_min", "s_max", "s_bfe", "s_bfm", "s_cselect", "s_cmp", "s_bitcmp", "s_bcnt",
                 "s_ff0", "s_ff1", "s_flbit", "s_sext", "s_brev", "s_abs", "s_pack", "s_wqm", "s_bitset")
ASM_CLASSES = (
    ("lds-dma", ("global_load_lds_",)),                      # buffer_load ... lds is told apart by its modifier, in asm_class()
    ("vmem-load", ("buffer_load_", "global_load_")),
    ("vmem-store", ("buffer_store_", "global_store_")),
    ("ds", ("ds_read", "ds_write", "ds_load", "ds_store", "ds_bpermute", "ds_permute", "ds_swizzle")),
    ("s_nop", ("s_nop",)),
    ("s_waitcnt", ("s_waitcnt",)),
    ("barrier/priority", ("s_barrier", "s_setprio", "s_sleep")),
    ("mfma", ("v_mfma", "v_smfma")),
    ("valu", ("v_",)),
    ("salu", SALU_PREFIXES),
)
BRANCH = ("s_cbranch", "s_branch")
INDIRECT = ("s_setpc", "s_swappc", "s_call", "s_rfe", "s_cbranch_g_fork", "s_cbranch_i_fork", "s_cbranch_join")
NO_DEST = ("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_setreg", "s_waitcnt", "s_nop", "s_barrier", "s_setprio", "s_sleep", "s_endpgm")
CARRY_OUT = ("v_div_scale", "v_mad_u64_u32", "v_mad_i64_i32")    # besides *_co_*: the second operand is a scalar destination

Ins = collections.namedtuple("Ins", "text asm line")


def operands(op):
    p = op.split(None, 1)
    return [x.strip() for x in p[1].split(",")] if len(p) > 1 else []


def regs(text):
    out = set()
    for m in re.finditer(r"\b([vs])(\d+)\b|\b([vs])\[(\d+):(\d+)\]", text):
        if m.group(1):
            out.add((m.group(1), int(m.group(2))))
        else:
            out |= {(m.group(3), i) for i in range(int(m.group(4)), int(m.group(5)) + 1)}
    return out


def sregs(text):
    """scalar registers of an operand text: s<N>, s[a:b], vcc / vcc_lo / vcc_hi"""
    out = {r for r in regs(text) if r[0] == "s"}
    if re.search(r"\bvcc(_lo)?\b", text):
        out.add(("vcc", 0))
    if re.search(r"\bvcc(_hi)?\b", text):
        out.add(("vcc", 1))
    return out


def vregs(text):
    return {r for r in regs(text) if r[0] == "v"}


def is_dma(op):
    m = op.split()[0]
    return (m.startswith("buffer_load") or m.startswith("global_load")) and bool(re.search(r"\blds\b|_lds_", op))


def is_vmem(op):
    return op.split()[0].startswith(("buffer_", "global_", "flat_", "scratch_", "tbuffer_"))


def asm_class(op):
    if is_dma(op):
        return "lds-dma"
    m = op.split()[0]
    for name, prefixes in ASM_CLASSES:
        if m.startswith(prefixes):
            return name
    return None


def states(op):
    """wait states an instruction stands for between a producer and a consumer"""
    p = op.split()
    return int(p[1], 0) + 1 if p[0] == "s_nop" else 1


def dma_operand_overwrites(ins):
    """LDS-DMA instructions directly followed by an instruction that writes one of their operand registers (hipcc does not see
    inside the asm statement and keeps no distance of its own; glds16b's M0 restore used to stand there)"""
    return len(dma_overwrite_sites(ins))


def dma_overwrite_sites(ins):
    hits = []
    for k, (a, b) in enumerate(zip(ins, ins[1:])):
        if not is_dma(a):
            continue
        m = b.split()[0]
        if m.startswith(("s_cmp", "s_bitcmp", "s_cbranch", "s_branch", "s_waitcnt", "s_nop", "s_barrier", "buffer_store", "global_store", "ds_write", "ds_store")):
            continue
        ops = operands(b)
        if ops and regs(ops[0]) & regs(a.split(None, 1)[1]):
            hits.append(k)
    return hits


# ---- what an instruction writes ---------------------------------------------------------------------------------------------
def valu_scalar_writes(op):
    """SGPRs / VCC halves a VALU instruction writes"""
    m = op.split()[0]
    if not m.startswith("v_"):
        return set()
    ops = operands(op)
    out = sregs(ops[0]) if ops else set()
    if len(ops) > 1 and ("_co_" in m or m.startswith(CARRY_OUT)):
        out |= sregs(ops[1])
    return out


def valu_vector_writes(op):
    m = op.split()[0]
    if not m.startswith("v_"):
        return set()
    ops = operands(op)
    out = vregs(ops[0]) if ops else set()
    if m.startswith("v_swap") and len(ops) > 1:
        out |= vregs(ops[1])
    return out


def writes_m0(op):
    m = op.split()[0]
    ops = operands(op)
    return bool(ops) and ops[0] == "m0" and m.startswith("s_") and not m.startswith(NO_DEST)


# ---- operand shapes of the VMEM forms that occur in asm ---------------------------------------------------------------------
V = r"v(?:\d+|\[\d+:\d+\])"
S4 = r"s\[\d+:\d+\]"
SOFF = r"(?:s\d+|m0|vcc_lo|vcc_hi|-?\d+|0x[0-9a-fA-F]+)"
SADDR = r"(?:off|s\[\d+:\d+\])"
MODS = r"(?:\s+(?:offen|idxen|lds|sc0|sc1|nt|glc|slc|offset:\d+|offset:-\d+))*"
SHAPES = (   # (mnemonic regex, operand regex with the named groups data / scalar)
    (r"buffer_load_\w+", rf"(?:off|{V}),\s*(?P<s1>{S4}),\s*(?P<s2>{SOFF}){MODS}"),                      # ... lds: no data operand
    (r"buffer_load_\w+", rf"(?P<dst>{V}),\s*(?:off|{V}),\s*(?P<s1>{S4}),\s*(?P<s2>{SOFF}){MODS}"),
    (r"buffer_store_\w+", rf"(?P<data>{V}),\s*(?:off|{V}),\s*(?P<s1>{S4}),\s*(?P<s2>{SOFF}){MODS}"),
    (r"global_load_lds_\w+", rf"{V},\s*(?P<s1>{SADDR}){MODS}"),
    (r"global_load_\w+", rf"(?P<dst>{V}),\s*{V},\s*(?P<s1>{SADDR}){MODS}"),
    (r"global_store_\w+", rf"{V},\s*(?P<data>{V}),\s*(?P<s1>{SADDR}){MODS}"),
    (r"flat_store_\w+", rf"{V},\s*(?P<data>{V}){MODS}"),
)


def vmem_parse(op):
    """{'scalar': registers read as descriptor / soffset / saddr, 'data': store-data VGPRs} or None if the form is not known"""
    p = op.split(None, 1)
    if len(p) < 2:
        return None
    for mre, ore in SHAPES:
        if re.fullmatch(mre, p[0]):
            m = re.fullmatch(ore, p[1].strip())
            if m:
                g = m.groupdict()
                return {"scalar": sregs(" ".join(g.get(k) or "" for k in ("s1", "s2"))), "data": vregs(g.get("data") or ""),
                        "m0": g.get("s2") == "m0"}
    return None


def store_width(op):
    m = re.match(r"(?:buffer|global|flat)_store_dwordx([34])\b", op)
    return int(m.group(1)) if m else 0


# ---- listing -> kernels -----------------------------------------------------------------------------------------------------
def kernels(src):
    """[[name, [Ins], {label: instruction index}, is a kernel]] for every function `_Z...:` up to its .Lfunc_end / .amdhsa_kernel"""
    out, cur, asm = [], None, False
    for n, l in enumerate(src, 1):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            cur = [m.group(1), [], {}, False]
            out.append(cur)
            asm = False
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\w+)", l)
        if m:
            for f in out:
                f[3] |= f[0] == m.group(1)
            cur = None
        if l.startswith(".Lfunc_end"):
            cur = None
        if cur is None:
            continue
        s = l.strip()
        if s.startswith(";;#ASMSTART"):
            asm = True
            continue
        if s.startswith(";;#ASMEND"):
            asm = False
            continue
        m = re.match(r"^(\.L\w+):", l)
        if m:
            cur[2][m.group(1)] = len(cur[1])
            continue
        t = s.split(";")[0].strip()
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        cur[1].append(Ins(t, asm, n))
    return out


def cfg(ins, labels):
    n = len(ins)
    succ, pred = [[] for _ in range(n)], [[] for _ in range(n)]
    for i, x in enumerate(ins):
        m = x.text.split()[0]
        nxt = []
        if m.startswith(BRANCH):
            t = labels.get(x.text.split()[1])
            if t is not None and t < n:
                nxt.append(t)
            if m.startswith("s_cbranch") and i + 1 < n:
                nxt.append(i + 1)
        elif m != "s_endpgm" and not m.startswith(("s_setpc", "s_rfe")) and i + 1 < n:     # (a call comes back behind itself)
            nxt.append(i + 1)
        for t in nxt:
            succ[i].append(t)
            pred[t].append(i)
    return succ, pred


def nearest(ins, edges, start, hit, need, opaque_end):
    """(fewest wait states between `start` and an instruction with hit(text) along `edges` (pred or succ) over all paths, its index)
    or None if every path collects need + HORIZON states or ends first; a path ends at its first hit.  Second result: True if a
    path met a call / return -- or, with opaque_end, ran out of the function -- with fewer than `need` states: not judged."""
    best, seen, undecided, limit = None, {}, False, need + HORIZON
    stack = [(j, 0) for j in edges[start]] or [(None, 0)]
    while stack:
        i, acc = stack.pop()
        if i is None or ins[i].text.split()[0].startswith(INDIRECT):
            undecided |= acc < need and (i is not None or opaque_end)
            continue
        if acc >= limit or (best is not None and acc >= best[0]) or seen.get(i, limit) <= acc:
            continue
        seen[i] = acc
        if hit(ins[i].text):
            best = (acc, i)
            continue
        acc += states(ins[i].text)
        stack.extend([(j, acc) for j in edges[i]] or [(None, acc)])
    return best, undecided


def audit(src):
    rep = {"kernels": 0, "functions": 0, "asm_blocks": sum(1 for l in src if l.strip().startswith(";;#ASMSTART")), "asm_vmem": collections.Counter(),
           "asm_vmem_judged": 0, "asm_classes": collections.Counter(), "unclassified": [], "unparsed": [], "calls_and_returns": [], "undecided": [],
           "rules": {"R1": {"need": 5, "judged": 0, "violations": [], "slack": collections.Counter()},
                     "R2": {"need": 1, "judged": 0, "violations": [], "slack": collections.Counter()},
                     "R3": {"need": 2, "judged": 0, "below_1": [], "below_2": [], "slack": collections.Counter()},
                     "R4": {"judged": 0, "violations": [], "m0_written_next": 0}}}
    R = rep["rules"]

    def site(name, x, other, st):
        return {"kernel": name, "line": x.line, "at": x.text, "other_line": other.line, "other": other.text, "states": st}

    def slack(rule, found):
        R[rule]["slack"]["far" if found is None else str(found[0] - NEED[rule])] += 1

    def near(rule, x, ins, edges, i, hit, need, opaque_end):
        best, undecided = nearest(ins, edges, i, hit, need, opaque_end)
        if undecided:
            rep["undecided"].append({"rule": rule, "kernel": name, "line": x.line, "at": x.text})
        return best

    for name, ins, labels, is_kernel in kernels(src):
        rep["kernels"] += is_kernel
        rep["functions"] += not is_kernel
        succ, pred = cfg(ins, labels)
        for x in ins:
            if x.text.split()[0].startswith(INDIRECT):
                rep["calls_and_returns"].append({"kernel": name, "line": x.line, "at": x.text})
        for i, x in enumerate(ins):
            op = x.text
            if x.asm:
                c = asm_class(op)
                rep["asm_classes"][c or "unclassified"] += 1
                if c is None:
                    rep["unclassified"].append({"kernel": name, "line": x.line, "at": op})
            if x.asm and is_vmem(op):
                form = op.split()[0] + (" lds" if is_dma(op) and op.startswith("buffer") else "")
                rep["asm_vmem"][form] += 1
                p = vmem_parse(op)
                if p is None:
                    rep["unparsed"].append({"kernel": name, "line": x.line, "at": op})
                else:
                    rep["asm_vmem_judged"] += 1
                    R["R1"]["judged"] += 1
                    if p["scalar"]:
                        f = near("R1", x, ins, pred, i, lambda t, want=p["scalar"]: bool(valu_scalar_writes(t) & want), 5, not is_kernel)
                        slack("R1", f)
                        if f is not None and f[0] < 5:
                            R["R1"]["violations"].append(site(name, x, ins[f[1]], f[0]))
                    else:
                        R["R1"]["slack"]["no scalar operand"] += 1
            if is_dma(op):
                R["R2"]["judged"] += 1
                f = near("R2", x, ins, pred, i, writes_m0, 1, not is_kernel)
                slack("R2", f)
                if f is not None and f[0] < 1:
                    R["R2"]["violations"].append(site(name, x, ins[f[1]], f[0]))
            if store_width(op):
                p = vmem_parse(op)
                if p is None:
                    if not x.asm:
                        rep["unparsed"].append({"kernel": name, "line": x.line, "at": op})
                    continue
                R["R3"]["judged"] += 1
                f = near("R3", x, ins, succ, i, lambda t, want=p["data"]: bool(valu_vector_writes(t) & want), 2, False)
                slack("R3", f)
                if f is not None and f[0] < 2:
                    R["R3"]["below_2"].append(site(name, x, ins[f[1]], f[0]))
                    if f[0] < 1:
                        R["R3"]["below_1"].append(site(name, x, ins[f[1]], f[0]))
        texts = [x.text for x in ins]
        R["R4"]["judged"] += sum(is_dma(t) for t in texts)
        for k in dma_overwrite_sites(texts):
            R["R4"]["violations"].append(site(name, ins[k], ins[k + 1], 0))
        R["R4"]["m0_written_next"] += sum(is_dma(a) and writes_m0(b) for a, b in zip(texts, texts[1:]))
    return rep


def failed(rep):
    R = rep["rules"]
    return bool(rep["unclassified"] or rep["unparsed"] or rep["undecided"] or R["R1"]["violations"] or R["R2"]["violations"]
                or R["R3"]["below_2"] or R["R4"]["violations"])


def hist(c):
    key = lambda k: (1, 0) if not k.lstrip("-").isdigit() else (0, int(k))
    return ", ".join(f"{k}: {c[k]}" for k in sorted(c, key=key)) or "-"


def by_kernel(sites):
    return sorted(collections.Counter(s["kernel"] for s in sites).items())


def report(rep):
    R = rep["rules"]
    out = [f"kernels {rep['kernels']} + {rep['functions']} device function(s); asm blocks {rep['asm_blocks']}; VMEM instructions inside asm blocks {sum(rep['asm_vmem'].values())}, "
           f"judged {rep['asm_vmem_judged']}:"]
    out += [f"  {k:32s} {v:6d}" for k, v in sorted(rep["asm_vmem"].items(), key=lambda kv: -kv[1])]
    out.append("instructions inside asm blocks by class: " + ", ".join(f"{k} {v}" for k, v in sorted(rep["asm_classes"].items())))
    out.append(f"unclassified asm mnemonics {len(rep['unclassified'])}; asm VMEM with unreadable operands {len(rep['unparsed'])}; "
               f"sites with a call / return inside their window (not judged) {len(rep['undecided'])}; calls and returns in all {len(rep['calls_and_returns'])}")
    out.append("")
    out.append(f"{'rule':5s} {'producer -> consumer':58s} {'need':>4s} {'sites':>6s} {'viol.':>6s}  source")
    rows = (("R1", "VALU writes SGPR/VCC -> asm buffer_/global_ reads it", 5, len(R["R1"]["violations"]), "GFX9 hazard table; og_kernels.hpp, og_buffer_store16"),
            ("R2", "SALU writes M0 -> LDS-DMA", 1, len(R["R2"]["violations"]), "GFX9 hazard table; og_kernels.hpp, glds16 / glds16b_m0"),
            ("R3", "16/12-byte store -> VALU writes its data VGPRs (< 1 state)", 1, len(R["R3"]["below_1"]), "GFX9 hazard table; og_kernels.hpp, og_buffer_store16"),
            ("R3", "16/12-byte store -> VALU writes its data VGPRs (< 2 states)", 2, len(R["R3"]["below_2"]), "gfx940 family (an asm store ends with s_nop 1); DESIGN 14"),
            ("R4", "LDS-DMA -> next instruction writes an operand register", "-", len(R["R4"]["violations"]), "og_kernels.hpp, glds16b_m0<PAD>"))
    for r, what, need, v, srcs in rows:
        out.append(f"{r:5s} {what:58s} {need!s:>4s} {R[r]['judged']:6d} {v:6d}  {srcs}")
    out.append("")
    out.append(f"slack = wait states present - needed, nearest producer over all paths; far = none within need + {HORIZON} states")
    for r in ("R1", "R2", "R3"):
        out.append(f"  {r} (need {NEED[r]}): {hist(R[r]['slack'])}")
    out.append(f"  R4: LDS-DMAs directly followed by a write of M0 (the restore of glds16 / glds16b; no violation): {R['R4']['m0_written_next']}")
    for r, key in (("R1", "violations"), ("R2", "violations"), ("R3", "below_2"), ("R4", "violations")):
        for k, n in by_kernel(R[r][key]):
            out.append(f"  {r} {key}: {n:4d} in {k}")
    for key in ("unclassified", "unparsed", "undecided"):
        for s in rep[key][:20]:
            out.append(f"  {key}: line {s['line']}: {s['at']}   ({s['kernel']})")
    return "\n".join(out)


def main():
    rep = audit(open(sys.argv[1]).read().split("\n"))
    print(json.dumps(rep) if "--json" in sys.argv else report(rep))
    sys.exit(1 if failed(rep) else 0)


if __name__ == "__main__":
    main()
