"""Static instruction audit of the tile end of k_conv_wino<1> and <2>: everything a wave issues behind the LAST MFMA of the
kernel -- the output transform Y = A^T M A on register pairs and the copies of wino_tile_end (one per combination of activation,
pooled output and fused head; a tile runs ONE of them).  The kernel runs one wave per SIMD and nothing overlaps a tile's end, so
every instruction here is paid in full, once per tile.  Prints one table row per instantiation and, per copy, what the copy holds.
usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only openglottal_amd/csrc/og_api.hip -o /tmp/api.s
       python tools/isa_wino_tail.py /tmp/api.s [--json]"""
import collections, json, os, re, sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_wino_loop import BRANCH, function, kind   # noqa: E402

COUNTED = ("v_accvgpr_read_b32", "v_pk_add_f32", "v_mov_b32", "v_pk_fma_f32", "v_max_f32", "buffer_store_dwordx4", "s_nop", "s_mul_i32",
           "s_waitcnt")


def mnem(op):
    """mnemonic without the encoding suffix hipcc prints on VOP1 / VOP2 / VOPC instructions"""
    m = op.split()[0]
    for suf in ("_e32", "_e64", "_sdwa", "_dpp"):
        if m.endswith(suf):
            return m[:-len(suf)]
    return m


def is_lds(op):
    return kind(op) in ("ds_read", "ds_write")


def blocks_of(ins, labels, lo):
    """basic blocks of ins[lo:]: a block starts at every label and behind every branch"""
    cuts = {lo, len(ins)} | {p for p in labels.values() if p > lo} | {k + 1 for k in range(lo, len(ins)) if ins[k].startswith(BRANCH)}
    cuts = sorted(cuts)
    return [(a, b) for a, b in zip(cuts, cuts[1:]) if b > a]


def audit(src, nt):
    ins, labels, meta = function(src, f"_Z11k_conv_winoILi{nt}EEv8ConvArgs")
    last = max(k for k, o in enumerate(ins) if kind(o) == "mfma")
    tail = ins[last + 1:]
    cnt = collections.Counter(mnem(o) for o in tail)
    kinds = collections.Counter(kind(o) for o in tail)
    r = {"kernel": f"k_conv_wino<{nt}>", **meta, "total": len(tail), "branch": kinds.get("branch", 0), "salu": kinds.get("salu", 0),
         "ds_read": kinds.get("ds_read", 0), "ds_write": kinds.get("ds_write", 0), **{m: cnt.get(m, 0) for m in COUNTED}}
    # moves that copy one VGPR into another (pairing registers up for a packed instruction), as opposed to constants and SGPRs
    r["v_mov_b32_from_vgpr"] = sum(1 for o in tail if re.match(r"v_mov_b32\S* v\d+, v\d+\b", o))
    # a 16-byte activation store and the wait state behind it (og_buffer_store16)
    r["store16_without_nop"] = sum(1 for k, o in enumerate(tail) if o.startswith("buffer_store_dwordx4")
                                   and not (k + 1 < len(tail) and tail[k + 1].startswith("s_nop")))
    # Copies of the tile end = the basic blocks that hold its LDS transposition.  A block has no branch inside and no branch target
    # but its first instruction, so "no branch into (or out of) a sub-tile step" is "every such block holds a WHOLE tile end":
    # the read-back of all four sub-tiles, 4 x 4 ds_read_b128 (+ 4 of the pooled tiles).
    copies = []
    outside = collections.Counter()
    for a, b in blocks_of(ins, labels, last + 1):
        blk = ins[a:b]
        c = collections.Counter(mnem(o) for o in blk)
        if any(is_lds(o) for o in blk) or c.get("buffer_store_dwordx4", 0):
            copies.append({"instructions": len(blk), "ds_read_b128": c.get("ds_read_b128", 0), "ds_write": sum(kind(o) == "ds_write" for o in blk),
                           "store16": c.get("buffer_store_dwordx4", 0), "store_other": sum(o.startswith("buffer_store") for o in blk) - c.get("buffer_store_dwordx4", 0),
                           "v_pk_add_f32": c.get("v_pk_add_f32", 0), "v_pk_fma_f32": c.get("v_pk_fma_f32", 0), "v_max_f32": c.get("v_max_f32", 0),
                           "v_mov_b32": c.get("v_mov_b32", 0), "v_accvgpr_read_b32": c.get("v_accvgpr_read_b32", 0), "s_mul_i32": c.get("s_mul_i32", 0),
                           "salu": sum(kind(o) == "salu" for o in blk), "s_waitcnt": c.get("s_waitcnt", 0)})
        else:
            outside.update(c)
    r["copies"] = copies
    r["split_copies"] = sum(1 for c in copies if c["ds_read_b128"] not in (16, 20))
    r["outside_copies"] = {m: outside.get(m, 0) for m in ("v_accvgpr_read_b32", "v_pk_add_f32", "v_mov_b32", "s_mul_i32")}
    return r


def main():
    src = open(sys.argv[1]).read().split("\n")
    rows = [audit(src, nt) for nt in (2, 1)]
    if "--json" in sys.argv:
        print(json.dumps(rows))
        return
    cols = ("total",) + COUNTED + ("ds_read", "ds_write", "salu", "branch")
    short = {"v_accvgpr_read_b32": "acc_read", "buffer_store_dwordx4": "store16"}
    print(f"{'behind the last MFMA':20s} " + " ".join(f"{short.get(c, c):>12s}" for c in cols))
    for r in rows:
        print(f"{r['kernel']:20s} " + " ".join(f"{r[c]:12d}" for c in cols))
    for r in rows:
        print(f"{r['kernel']}: VGPRs {r['vgprs']} AGPRs {r['agprs']} scratch {r['scratch']}; 16-byte stores without a wait state behind them "
              f"{r['store16_without_nop']}; v_mov_b32 that copy a VGPR {r['v_mov_b32_from_vgpr']}; copies of the tile end {len(r['copies'])}, of them split by a branch or a branch target {r['split_copies']}; "
              f"outside the copies (transform + choice of the copy + set-up): {r['outside_copies']}")
        for i, c in enumerate(r["copies"]):
            print(f"  copy {i}: " + " ".join(f"{k}={v}" for k, v in c.items()))


if __name__ == "__main__":
    main()
