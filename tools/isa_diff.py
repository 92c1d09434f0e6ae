"""Two hipcc -S listings of the shipped device code, symbol by symbol: what a refactor of the kernels' SOURCE may not change.

Byte identity is too strict a bar for a source refactor (a moved expression changes a compare form or a shift in the set-up code)
and "same results" too loose (a lost register or an extra LDS read costs speed first).  Per symbol this prints

  HARD  the same symbols on both sides, each with equal NumVgprs, NumAgprs, NumSgprs, ScratchSize, LDS size and Occupancy;
  HARD  the same ordered sequence of mnemonics over v_mfma* / ds_* / buffer_* / global_* / s_waitcnt / s_barrier
        (compiler-inserted s_nop is not part of it);
  HARD  tools/isa_hazards.py judges as many asm VMEM sites on both sides and finds no violation on either;
  TARGET every basic block that holds an MFMA is identical up to register numbers and label names; each exception is printed
        with its diff.

and classifies every symbol: `identical` (byte for byte), `renamed` (identical up to register numbers and labels), `set-up`
(differs outside the MFMA blocks only), `MFMA-BLOCK` (a target exception), `HARD` (fails a hard check).  "Up to register numbers"
= every v / s / a register or range is replaced by its class and width, every label by a placeholder.

usage: python tools/isa_diff.py parent.s branch.s [--no-hazards]     exit code 1 on any HARD failure, 2 on target exceptions only"""
import collections, difflib, os, re, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_hazards as H  # noqa: E402

RESOURCES = (("NumVgprs", r"; NumVgprs: (\d+)"), ("NumAgprs", r"; NumAgprs: (\d+)"), ("NumSgprs", r"; (?:Total)?NumSgprs: (\d+)"),
             ("ScratchSize", r"; ScratchSize: (\d+)"), ("LDS", r"; LDSByteSize: (\d+)"), ("Occupancy", r"; Occupancy: (\d+)"))
SEQ = ("v_mfma", "ds_", "buffer_", "global_", "s_waitcnt", "s_barrier")
BRANCH = ("s_cbranch", "s_branch", "s_endpgm", "s_setpc", "s_swappc")

Sym = collections.namedtuple("Sym", "ins res blocks")


def normalise(text):
    text = re.sub(r"\b([vsa])\[(\d+):(\d+)\]", lambda m: f"{m.group(1)}[#{int(m.group(3)) - int(m.group(2)) + 1}]", text)
    text = re.sub(r"\b([vsa])\d+\b", r"\1#", text)
    return re.sub(r"\.L\w+", ".L#", text)


def symbols(src):
    """{name: Sym(instruction texts, {resource: value}, basic blocks as lists of instruction texts)}"""
    res, name = {}, None
    for l in src:
        m = re.match(r"^(_Z\w+):", l)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        if name:
            for key, pat in RESOURCES:
                m = re.match(pat, l)
                if m:
                    res[name].setdefault(key, int(m.group(1)))
    out = {}
    for name, ins, labels, _ in H.kernels(src):
        starts = set(labels.values()) | {0}
        blocks, cur = [], []
        for i, x in enumerate(ins):
            if i in starts and cur:
                blocks.append(cur)
                cur = []
            cur.append(x.text)
            if x.text.split()[0].startswith(BRANCH):
                blocks.append(cur)
                cur = []
        if cur:
            blocks.append(cur)
        out[name] = Sym([x.text for x in ins], res.get(name, {}), blocks)
    return out


def mem_sequence(ins):
    return [t.split()[0] for t in ins if t.split()[0].startswith(SEQ)]


def mfma_blocks(sym):
    return [[normalise(t) for t in b] for b in sym.blocks if any(t.startswith("v_mfma") for t in b)]


def compare(a, b):
    """rows [(name, class, note)], exceptions [(name, block number, unified diff)] for two symbols() results"""
    rows, exceptions = [], []
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            rows.append((name, "HARD", "only in the " + ("second" if name in b else "first") + " listing"))
            continue
        x, y = a[name], b[name]
        hard = [f"{k} {x.res.get(k)} -> {y.res.get(k)}" for k, _ in RESOURCES if x.res.get(k) != y.res.get(k)]
        sx, sy = mem_sequence(x.ins), mem_sequence(y.ins)
        if sx != sy:
            d = [l for l in difflib.unified_diff(sx, sy, lineterm="", n=0) if l[0] in "+-" and l[:3] not in ("+++", "---")]
            hard.append(f"memory / MFMA / wait sequence {len(sx)} -> {len(sy)} entries: " + " ".join(d[:6]) + (" ..." if len(d) > 6 else ""))
        note = f"{len(x.ins)} -> {len(y.ins)} instructions"
        if hard:
            rows.append((name, "HARD", "; ".join(hard)))
        elif x.ins == y.ins:
            rows.append((name, "identical", f"{len(x.ins)} instructions"))
        elif [normalise(t) for t in x.ins] == [normalise(t) for t in y.ins]:
            rows.append((name, "renamed", note))
        else:
            mx, my = mfma_blocks(x), mfma_blocks(y)
            bad = [k for k in range(max(len(mx), len(my))) if k >= len(mx) or k >= len(my) or mx[k] != my[k]]
            for k in bad:
                d = difflib.unified_diff(mx[k] if k < len(mx) else [], my[k] if k < len(my) else [], lineterm="", n=1)
                exceptions.append((name, k, "\n".join(d)))
            rows.append((name, "MFMA-BLOCK" if bad else "set-up", note + (f"; {len(bad)} of {len(mx)} MFMA blocks differ" if bad else f"; {len(mx)} MFMA blocks equal")))
    return rows, exceptions


def hazards(src):
    rep = H.audit(src)
    return rep["asm_vmem_judged"], H.failed(rep)


def main():
    pa, pb = [a for a in sys.argv[1:] if not a.startswith("--")]
    sa, sb = open(pa).read().split("\n"), open(pb).read().split("\n")
    rows, exceptions = compare(symbols(sa), symbols(sb))
    for name, cls, note in rows:
        print(f"{cls:10s} {name}\n           {note}")
    count = collections.Counter(cls for _, cls, _ in rows)
    print(f"\n{len(rows)} symbols: " + ", ".join(f"{count[c]} {c}" for c in ("identical", "renamed", "set-up", "MFMA-BLOCK", "HARD")))
    hard = count["HARD"] > 0
    if "--no-hazards" not in sys.argv:
        (na, fa), (nb, fb) = hazards(sa), hazards(sb)
        print(f"hazard audit (tools/isa_hazards.py): asm VMEM sites judged {na} -> {nb}; violations: first {'yes' if fa else 'none'}, second {'yes' if fb else 'none'}")
        hard |= na != nb or fa or fb
    for name, k, d in exceptions:
        print(f"\nMFMA block {k} of {name}:\n{d}")
    sys.exit(1 if hard else 2 if exceptions else 0)


if __name__ == "__main__":
    main()
