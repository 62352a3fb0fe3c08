"""Static report on the gfx950 ISA of the step kernel: where the vector issue slots of rr_step_kernel go that are not arithmetic.

Runs on the CPU.  Compiles csrc/rr_api.hip device-only to assembly with the flags of __graft_entry__.build() (read from its source,
so a change of the build flags is followed), then prints

  * for every rr_step_kernel instance: VGPRs, SGPRs, VGPR / SGPR spills, scratch and LDS (the code-object metadata that
    tools/kernel_meta.py reads from the library, here from the assembly's own metadata block);
  * for ONE instance (default: the instance the driver protocol times, the multi-step fixed-dimension rodent kernel):
      - its VALU instructions by class (float arithmetic / integer, address and other / v_cmp / v_cndmask / v_mov / lane operations /
        DPP) and its s_nop count;
      - by LLVM loop depth (the `Depth=` comments of the basic blocks; 1 = env-step loop, 2 = substep body, 3+ = solver loops and
        row programs): VALU instructions, SGPR-spill reload sites (v_readlane_b32 from a VGPR that v_writelane_b32 fills),
        64-bit address instructions, and table loads in the per-lane 64-bit form (`vaddr, off`) against the SGPR-base form;
      - the spill lanes with the most reload sites.

usage: python tools/isa_report.py [--asm FILE] [--keep-asm FILE] [--instance MANGLED_SUBSTRING] [--top N]
       --asm analyses an assembly file made earlier instead of compiling (about three minutes).
"""
import argparse
import ast
import collections
import os
import re
import subprocess
import sys
import tempfile

import yaml

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(HERE, "brax-rodent-run_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
# rr_step_kernel<2, 2, 1, false, false, RRDimsRodent, false, /*UNROLL*/ true, false, false, false>
TIMED = "rr_step_kernelILi2ELi2ELi1ELb0ELb0E11RRDimsFixedILi66ELi59ELi1263EELb0ELb1ELb0ELb0ELb0EE"


def build_flags():
    """The string literals of the `cmd = [...]` list in __graft_entry__.build(), minus what makes a shared library of them."""
    tree = ast.parse(open(os.path.join(HERE, "__graft_entry__.py")).read())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "build")
    for n in ast.walk(fn):
        if isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id == "cmd" for t in n.targets) and isinstance(n.value, ast.List):
            lits = [e.value for e in n.value.elts if isinstance(e, ast.Constant) and isinstance(e.value, str)]
            return [f for f in lits if f not in ("-shared", "-o")]
    raise RuntimeError("no `cmd = [...]` in __graft_entry__.build()")


def compile_asm(out):
    cmd = build_flags() + ["--cuda-device-only", "-S", "-o", out, os.path.join(CSRC, "rr_api.hip")]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    sys.stderr.write("".join(l for l in r.stderr.splitlines(True) if "not a recognized feature" not in l and "--hip-link" not in l))
    if r.returncode:
        raise subprocess.CalledProcessError(r.returncode, cmd)
    return cmd


def demangle(names):
    try:
        out = subprocess.run([os.path.join(LLVM, "llvm-cxxfilt")], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def metadata(text):
    """name -> the instance's entry of amdhsa.kernels (the metadata block at the end of the assembly is YAML)."""
    a = text.rindex(".amdgpu_metadata") + len(".amdgpu_metadata")
    doc = yaml.safe_load(text[a:text.rindex(".end_amdgpu_metadata")].replace("\t", " "))
    return {k[".name"]: {f[1:]: v for f, v in k.items() if isinstance(v, int)} for k in doc["amdhsa.kernels"]}


def kernel_blocks(text, name):
    """The instance's body as a list of (loop depth, [instruction lines])."""
    lines = text.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    blocks, depth, cur = [], 0, []
    i = start + 1
    while i < len(lines) and not lines[i].startswith(".Lfunc_end"):
        l = lines[i]
        if re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", l):        # a basic block: its header comment (and continuation lines) names the loop
            if cur:
                blocks.append((depth, cur))
            cur, hdr, j = [], [l], i + 1
            while j < len(lines) and re.match(r"\s+;", lines[j]):
                hdr.append(lines[j]); j += 1
            depth, own = 0, None
            for h in hdr:
                m = re.search(r"Depth=(\d+)", h)
                if not m:
                    continue
                if "=>" in h:
                    own = int(m.group(1))
                elif "in Loop:" in h:
                    depth = int(m.group(1))
            if own is not None:
                depth = own
            i = j
            continue
        s = l.strip()
        if s and not s.startswith((";", ".", "//")):
            cur.append(s.split(";")[0].strip())
        i += 1
    if cur:
        blocks.append((depth, cur))
    return blocks


FLOAT = re.compile(r"v_(pk_)?(add|sub|subrev|mul|mac|fma|fmac|fmaak|fmamk|mad|madak|madmk|max|min|max3|min3|med3|rcp|rsq|sqrt|exp|log|sin|cos|fract|floor|ceil|trunc|rndne|ldexp|"
                   r"frexp_mant|div_scale|div_fmas|div_fixup|mul_legacy|cvt)\w*_f(16|32|64)(_|$)|v_cvt_")


def valu_class(mn):
    if "_dpp" in mn:
        return "DPP"
    if mn.startswith("v_cmp") or mn.startswith("v_cmpx"):
        return "v_cmp*"
    if mn.startswith("v_cndmask"):
        return "v_cndmask*"
    if mn.startswith(("v_mov", "v_accvgpr")):
        return "v_mov*"
    if mn.startswith(("v_readlane", "v_writelane", "v_readfirstlane", "v_permlane", "v_swap")):
        return "lane operations"
    if FLOAT.match(mn) and not mn.startswith("v_cvt_"):
        return "float arithmetic (packed included)"
    return "integer / address / conversions / other"


ADDR64 = ("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_addc_co_u32", "v_lshlrev_b64", "v_add_u64")


def report(text, name, top, out):
    blocks = kernel_blocks(text, name)
    insts = [(d, s) for d, b in blocks for s in b]
    spill_regs = set()
    for _, s in insts:
        m = re.match(r"v_writelane_b32 (v\d+), s\d+, \d+", s)
        if m:
            spill_regs.add(m.group(1))
    cls = collections.Counter()
    by_depth = collections.defaultdict(collections.Counter)
    lanes = collections.Counter()
    lane_depth = collections.defaultdict(collections.Counter)
    writes_head = 0
    for d, s in insts:
        mn = s.split()[0]
        c = by_depth[d]
        if mn.startswith("s_nop"):
            cls["s_nop"] += 1
        if mn.startswith("s_load") or mn.startswith("s_buffer_load"):
            c["scalar loads"] += 1
        if mn.startswith("s_waitcnt"):
            c["s_waitcnt"] += 1
        if mn.startswith("v_"):
            cls[valu_class(mn)] += 1
            c[valu_class(mn)] += 1
            cls["VALU"] += 1
            c["VALU"] += 1
            m = re.match(r"v_readlane_b32 s\d+, (v\d+), (\d+)", s)
            if m and m.group(1) in spill_regs:
                c["spill reloads"] += 1
                lanes[(m.group(1), int(m.group(2)))] += 1
                lane_depth[(m.group(1), int(m.group(2)))][d] += 1
            if mn == "v_writelane_b32":
                c["spill writes"] += 1
                writes_head += d == 0
            if mn in ADDR64 or (mn == "v_ashrrev_i32_e32" and re.match(r"v_ashrrev_i32_e32 v\d+, 31,", s)):
                c["64-bit address VALU"] += 1
                cls["of all classes: 64-bit address (" + mn.replace("_e32", "") + ")"] += 1
        if mn.startswith("global_load"):
            ops = s[len(mn):].split(",")
            saddr = len(ops) >= 3 and ops[2].strip().startswith("s[")
            c["table loads, SGPR base"] += saddr
            c["table loads, 64-bit vaddr"] += not saddr
        if mn.startswith("flat_load"):
            c["flat loads"] += 1
        if mn.startswith("scratch_"):
            c["scratch accesses"] += 1
    p = lambda *a: print(*a, file=out)
    p("instance: %s" % name)
    p("  static VALU instructions: %d; s_nop: %d" % (cls["VALU"], cls["s_nop"]))
    for k in ("float arithmetic (packed included)", "integer / address / conversions / other", "v_cmp*", "v_cndmask*", "v_mov*", "lane operations", "DPP"):
        p("    %-42s %6d  %5.1f %%" % (k, cls[k], 100.0 * cls[k] / max(cls["VALU"], 1)))
    for k in sorted(k for k in cls if k.startswith("of all classes")):
        p("    %-62s %6d" % (k, cls[k]))
    p("  VGPRs that hold spilled SGPRs: %s; v_writelane_b32 in all: %d, of them ahead of the first loop: %d"
      % (" ".join(sorted(spill_regs)) or "none", sum(c["spill writes"] for c in by_depth.values()), writes_head))
    p("  by loop depth (0 = outside every loop, 1 = env-step loop, 2 = substep body, 3+ = solver loops / row programs):")
    cols = ("VALU", "spill reloads", "spill writes", "64-bit address VALU", "table loads, 64-bit vaddr", "table loads, SGPR base", "scalar loads", "s_waitcnt",
            "flat loads", "scratch accesses")
    p("    depth " + " ".join("%24s" % c for c in cols))
    for d in sorted(by_depth):
        p("    %5d " % d + " ".join("%24d" % by_depth[d][c] for c in cols))
    p("  VALU classes by loop depth:")
    kl = ("float arithmetic (packed included)", "integer / address / conversions / other", "v_cmp*", "v_cndmask*", "v_mov*", "lane operations", "DPP")
    p("    depth " + " ".join("%40s" % k for k in kl))
    for d in sorted(by_depth):
        p("    %5d " % d + " ".join("%40d" % by_depth[d][k] for k in kl))
    for d in sorted(by_depth):
        tl = by_depth[d]["table loads, 64-bit vaddr"] + by_depth[d]["table loads, SGPR base"]
        if tl:
            p("    depth %d: %.1f %% of %d table loads in the SGPR-base form" % (d, 100.0 * by_depth[d]["table loads, SGPR base"] / tl, tl))
    p("  spill-reload sites at depth >= 3: %d" % sum(c["spill reloads"] for d, c in by_depth.items() if d >= 3))
    p("  most-reloaded spill lanes (register[lane]: reload sites, by depth):")
    for (r, l), n in lanes.most_common(top):
        p("    %s[%2d]: %3d   %s" % (r, l, n, " ".join("d%d:%d" % (d, k) for d, k in sorted(lane_depth[(r, l)].items()))))
    return cls, by_depth


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--asm", help="assembly file made earlier (skips the compile)")
    ap.add_argument("--keep-asm", help="where to leave the assembly of this run")
    ap.add_argument("--instance", default=TIMED, help="substring of the mangled name of the instance to break down")
    ap.add_argument("--top", type=int, default=16)
    a = ap.parse_args()
    tmp = None
    if a.asm:
        path = a.asm
        print("assembly: %s (made earlier)" % os.path.basename(path))
    else:
        if a.keep_asm:
            path = a.keep_asm
        else:
            tmp = tempfile.mkdtemp(prefix="rr_isa_")
            path = os.path.join(tmp, "rr_api.s")
        cmd = compile_asm(path)
        print("compiled with: " + " ".join(os.path.relpath(c, HERE) if os.path.isabs(c) and c.startswith(HERE) else c for c in cmd[:-3]))
    text = open(path).read()
    meta = metadata(text)
    names = sorted(n for n in meta if "rr_step_kernel" in n)
    dm = demangle(names)
    print("rr_step_kernel instances (template arguments NBS, NVS, NCS, PROF, DBG, dims, NEWTON, UNROLL, ACTOR, PAIR, DYN):")
    for n in names:
        k = meta[n]
        short = re.sub(r"^void rr_step_kernel<(.*)>\(.*$", r"\1", dm[n]).replace("RRDimsFixed<66, 59, 1263>", "RRDimsRodent").replace("RRDimsFixed<67, 57, 1279>", "RRDimsRodentNew")
        print("  %-78s vgpr %3d agpr %3d sgpr %3d  spills v %3d s %3d  scratch %4d B  lds %5d B"
              % (short, k.get("vgpr_count", -1), k.get("agpr_count", 0), k.get("sgpr_count", -1), k.get("vgpr_spill_count", 0),
                 k.get("sgpr_spill_count", 0), k.get("private_segment_fixed_size", -1), k.get("group_segment_fixed_size", -1)))
    hit = [n for n in names if a.instance in n]
    if len(hit) != 1:
        sys.exit("--instance matches %d instances" % len(hit))
    print()
    report(text, hit[0], a.top, sys.stdout)
    if tmp:
        import shutil
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
