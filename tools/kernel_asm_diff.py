"""Compare two device-only `-S` outputs of csrc/rr_api.hip kernel by kernel: did a source change move any instruction?

Each file is `hipcc <build()'s flags> --cuda-device-only -S -o x.s csrc/rr_api.hip` of one tree.  Per kernel symbol the instruction
lines are taken (comments, directives and labels dropped, branch targets reduced to the block number, the file-wide counter of the
long branches' `.Lpost_getpc<n>` labels dropped) and compared:
  identical            the same instructions in the same order
  reordered            the same multiset of instructions in another order
  reordered, renamed   the same multiset of opcodes: another order and another register assignment
  differs (n -> m)     anything else, with the instruction counts
next to the registers, spills and scratch of both sides (the kernel descriptor and metadata in the assembly).

usage: python tools/kernel_asm_diff.py parent.s this.s
"""
import collections
import re
import sys


def kernels(path):
    """{symbol: (instructions, {vgpr, sgpr_spill, vgpr_spill, scratch})} of the kernels of one assembly file."""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.M | re.S):
        ins = []
        for line in m.group(2).split("\n"):
            line = line.split(";")[0].strip()
            if line and not line.startswith(".") and not line.endswith(":"):
                # labels numbered over the whole file, not per kernel: the function number in .LBB<f>_<block>, and the count of long
                # branches in .Lpost_getpc<n> -- both move when a kernel before this one is added or removed
                ins.append(re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", line))))
        out[m.group(1)] = [ins, {}]
    for m in re.finditer(r"^  - \.agpr_count:.*?(?=^  - \.agpr_count:|^amdhsa\.target)", text, re.M | re.S):      # one metadata entry per kernel
        f = lambda k: int(re.search(r"^\s+\.%s:\s+(\d+)" % k, m.group(0), re.M).group(1))
        name = re.search(r"^\s+\.name:\s+(\S+)", m.group(0), re.M).group(1)
        if name in out:
            out[name][1] = dict(vgpr=f("vgpr_count"), sgpr_spill=f("sgpr_spill_count"), vgpr_spill=f("vgpr_spill_count"), scratch=f("private_segment_fixed_size"))
    return out


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    tally = collections.Counter()
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            verdict = "only in " + (sys.argv[1] if name in a else sys.argv[2])
        else:
            (ia, ra), (ib, rb) = a[name], b[name]
            ops = lambda ins: collections.Counter(i.split()[0] for i in ins)
            verdict = "identical" if ia == ib else ("reordered" if collections.Counter(ia) == collections.Counter(ib) else
                                                    ("reordered, renamed" if ops(ia) == ops(ib) else f"differs ({len(ia)} -> {len(ib)} instructions)"))
            res = "  ".join(f"{k} {ra[k]}" + ("" if ra[k] == rb[k] else f" -> {rb[k]}") for k in ra)
            verdict = f"{verdict:40s} {res}"
        tally[verdict.split("(")[0].split("  ")[0].strip()] += 1
        print(f"{name:110s} {verdict}")
    print("# " + ", ".join(f"{n} {v}" for v, n in sorted(tally.items())))
