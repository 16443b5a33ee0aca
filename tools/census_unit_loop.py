"""Static census of a kernel's instruction stream along one path through its control-flow graph, from the disassembly of the
gfx950 code object (what one iteration of the dealt kernels' unit loop issues outside the k-loop).

    llvm-objdump -d --no-show-raw-insn dev.elf > dev.s
    census_unit_loop.py dev.s <kernel symbol substring>                    the kernel's basic blocks, one line each
    census_unit_loop.py dev.s <kernel symbol substring> <b0> <b1> ...      the instructions of that path of blocks, by class

A block is named by the number the first form prints; x<number> walks a block without counting it (the k-loop).  The path is chosen by hand from the listing (the branch a finite,
fast-sigmoid, two-tile, non-counting unit takes at every fork); the second form checks that each block can follow the one before it.
Classes: mfma; valu_int (integer / bit / move / lane instructions of the vector ALU); valu_fp; lds; vmem; salu (everything scalar,
branches and waits included)."""
import re
import sys
from collections import Counter


def classify(op):
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("v_"):
        fp = re.search(r"_(f16|f32|f64|bf16)", op) and not op.startswith(("v_cvt", "v_cmp", "v_cmpx", "v_cndmask"))
        return "valu_fp" if fp else "valu_int"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return "salu"


def load(path, sym):
    ins, on = [], False
    for line in open(path):
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            if on:
                break
            on = sym in m.group(1)
            continue
        if on:
            m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
            if m:
                ins.append((int(m.group(3), 16), m.group(1), m.group(2)))
    assert ins, f"no kernel matches {sym}"
    return ins


def blocks_of(ins):
    addr_index = {a: i for i, (a, _, _) in enumerate(ins)}
    leaders, edges = {0}, {}
    for i, (a, op, args) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")):
            off = int(args.split()[0])
            off = off - 65536 if off >= 32768 else off
            t = addr_index.get(a + 4 + 4 * off)
            edges[i] = (t, None if op == "s_branch" else i + 1)
            if t is not None:
                leaders.add(t)
            leaders.add(i + 1)
        elif op == "s_endpgm":
            edges[i] = (None, None)
            leaders.add(i + 1)
    starts = sorted(x for x in leaders if x < len(ins))
    number = {s: k for k, s in enumerate(starts)}
    out = []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(ins)
        succ = edges.get(e - 1, (None, e))
        out.append((s, e, [number.get(x) for x in succ if x is not None and x in number]))
    return out


def main():
    ins = load(sys.argv[1], sys.argv[2])
    blocks = blocks_of(ins)
    if len(sys.argv) == 3:
        for k, (s, e, succ) in enumerate(blocks):
            c = Counter(classify(op) for _, op, _ in ins[s:e])
            last = ins[e - 1]
            print(f"{k:4d} @{ins[s][0]:x} n={e - s:4d} mfma={c['mfma']:3d} vint={c['valu_int']:3d} vfp={c['valu_fp']:3d} lds={c['lds']:3d} "
                  f"vmem={c['vmem']:2d} salu={c['salu']:3d}  {last[1]} -> {succ}")
        return
    skipped = {i for i, a in enumerate(sys.argv[3:]) if a.startswith("x")}  # x<block>: on the path, not counted (the k-loop)
    path = [int(a.lstrip("x")) for a in sys.argv[3:]]
    total, ops = Counter(), Counter()
    for i, k in enumerate(path):
        s, e, succ = blocks[k]
        if i + 1 < len(path):
            assert path[i + 1] in succ, f"block {path[i + 1]} does not follow block {k} (successors {succ})"
        if i in skipped:
            continue
        for _, op, _ in ins[s:e]:
            total[classify(op)] += 1
            ops[op] += 1
    print(dict(total))
    for op, n in sorted(ops.items(), key=lambda kv: (classify(kv[0]), -kv[1])):
        print(f"  {classify(op):9s} {n:4d}  {op}")


if __name__ == "__main__":
    main()
