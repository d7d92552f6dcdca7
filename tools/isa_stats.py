#!/usr/bin/env python3
"""Per-kernel ISA statistics of one unit's device-only asm (kernels.hip, mv_*.hip, attn.hip): cross-lane op counts,
vmcnt(0) waits, VALU / v_mov_b32 / v_dot4* / s_nop counts, VGPRs, occupancy, scratch.
Usage: isa_stats.py k.s [name-filter]
       isa_stats.py k.s name-filter --blocks [N]  also the counts of every basic block with at least N (default 40)
                                               VALU instructions, in layout order, with the branch that ends it.  A
                                               block starts at a .LBB label or at a fall-through "; %bb.N:" comment
                                               (a unit block of k_matvec is the one with 64 or 128 v_dot4)"""
import re
import subprocess
import sys


def demangle(name):
    try:
        return subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return name


def ops(body):
    """mnemonics of the instruction lines of an asm body (labels, directives and comments dropped)"""
    out = []
    for ln in body.split("\n"):
        ln = ln.strip()
        if not ln or ln[0] in ".;" or ln.endswith(":"):
            continue
        out.append(ln.split()[0])
    return out


def counts(o):
    return (sum(x.startswith("v_") for x in o), sum(x.startswith("v_mov_b32") for x in o),
            sum(x.startswith("v_dot4") for x in o), sum(x == "s_nop" for x in o))


def main():
    argv = sys.argv[1:]
    blocks, bmin = "--blocks" in argv, 40
    if blocks:
        i = argv.index("--blocks")
        if i + 1 < len(argv) and argv[i + 1].isdigit():
            bmin = int(argv.pop(i + 1))
    args = [a for a in argv if not a.startswith("--")]
    s = open(args[0]).read()
    flt = args[1] if len(args) > 1 else "k_matvec"
    for m in re.finditer(r"\n(_ZN4llmi\w+):[^\n]*\n(.*?)\.Lfunc_end", s, re.S):
        name, body = m.groups()
        pretty = re.sub(r"^void llmi::|\(.*$", "", demangle(name))
        if flt not in name and flt not in pretty:
            continue
        tail = s[m.end():m.end() + 4000]
        vg = re.search(r"; NumVgprs: (\d+)", tail)
        occ = re.search(r"; Occupancy: (\d+)", tail)
        sp = re.search(r"; ScratchSize: (\d+)", tail)
        valu, vmov, vdot, snop = counts(ops(body))
        print(f"{pretty[:48]:48s} bperm {body.count('ds_bpermute'):3d} dpp {body.count('_dpp'):3d} "
              f"permlane {body.count('permlane'):3d} vmcnt0 {body.count('vmcnt(0)'):3d} instr {body.count(chr(10)):5d} "
              f"valu {valu:5d} v_mov {vmov:4d} v_dot4 {vdot:4d} s_nop {snop:4d} "
              f"vgpr {vg.group(1) if vg else '?'} occ {occ.group(1) if occ else '?'} scratch {sp.group(1) if sp else '?'}")
        if blocks:
            cur, lines = "entry", []

            def flush():
                valu, vmov, vdot, snop = counts(ops("\n".join(lines)))
                if valu >= bmin:
                    br = [ln.split()[0] + " " + ln.split()[1] for ln in lines if ln.startswith(("s_cbranch", "s_branch"))]
                    print(f"    {cur:14s} valu {valu:5d} v_mov {vmov:4d} v_dot4 {vdot:4d} s_nop {snop:4d}  {', '.join(br)}")

            for ln in body.split("\n"):
                ln = ln.strip()
                m2 = re.match(r"(\.LBB\w+):|; (%bb\.\d+):", ln)
                if m2:
                    flush()
                    cur, lines = m2.group(1) or m2.group(2), []
                else:
                    lines.append(ln)
            flush()

if __name__ == "__main__":
    main()
