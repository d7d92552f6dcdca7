#!/usr/bin/env python3
"""The entry chain of each kernel in a unit's device-only asm (hipcc -S --cuda-device-only with
the Makefile's FLAGS): how many dependent memory round trips a wave makes before its bulk
loads are in flight.  Per kernel:

  swaits   scalar-memory waits ahead of the first vector-memory load: s_waitcnt lines with an
           lgkmcnt field that have at least one s_load outstanding
  vmwaits  vmcnt waits between the first and the last vector-memory load: s_waitcnt lines with a
           vmcnt field that another vector-memory load follows (the wave stood still with
           loads left to issue).  For a kernel that issues every load at entry (the attention
           kernels) this is the entry block's count and should be 0; a kernel that loads in a
           loop (the matvecs) also counts its loop's waits here
  lead     vector-memory loads issued before the first vmcnt wait
  loads    vector-memory loads in the kernel
  preload  .amdhsa_user_sgpr_kernarg_preload_length: kernel-argument dwords that arrive in
           SGPRs with the wave

A kernel with preloaded arguments begins with the compiler's preamble for firmware without
preload (s_load of the same arguments, a wait, a branch over the padding to the 256-byte
boundary where preloading firmware enters): the lines before its .p2align are not counted.

The tool reads s_load*, s_waitcnt, global_load* / buffer_load*, the .amdhsa_* lines and the
.p2align of the preamble; nothing else of a kernel's body.

Usage: entry_chain.py k.s [name-filter ...]     (a kernel is listed when any filter matches
                                                 its mangled or demangled name; default all)"""
import re
import subprocess
import sys

KERNEL = re.compile(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", re.S | re.M)


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def _field(line, name):
    m = re.search(name + r"\((\d+)\)", line)
    return int(m.group(1)) if m else None


def entry_chain(body):
    """(swaits, vmwaits, lead, loads, preload) of one kernel's asm body (label to .Lfunc_end)."""
    m = re.search(r"\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", body)
    preload = int(m.group(1)) if m else 0
    lines = [ln.strip() for ln in body.split("\n")]
    if preload > 0:
        for i, ln in enumerate(lines):
            if ln.startswith(".p2align"):
                lines = lines[i + 1:]
                break
    swaits = vmwaits = loads = 0
    lead = None        # loads issued before the first vmcnt wait
    pending_s = 0      # s_loads issued since the last lgkmcnt wait
    pending_vm = 0     # vmcnt waits since the last vector load (counted once a load follows)
    for ln in lines:
        op = ln.split(None, 1)[0] if ln else ""
        if op.startswith("s_load"):
            pending_s += 1
        elif op.startswith(("global_load", "buffer_load")):
            loads += 1
            vmwaits += pending_vm
            pending_vm = 0
        elif op == "s_waitcnt":
            if not loads:
                if _field(ln, "lgkmcnt") is not None and pending_s:
                    swaits += 1
                    pending_s = 0
            elif _field(ln, "vmcnt") is not None:
                pending_vm += 1
                if lead is None:
                    lead = loads
    return swaits, vmwaits, loads if lead is None else lead, loads, preload


def kernels(text):
    return [(m.group(1), m.group(2)) for m in KERNEL.finditer(text) if ".amdhsa_kernel" in m.group(2)]


def main():
    args = sys.argv[1:]
    if not args:
        sys.exit(__doc__)
    ks = kernels(open(args[0]).read())
    pretty = demangle([n for n, _ in ks])
    for name, body in ks:
        p = re.sub(r"^void ", "", pretty[name])
        if args[1:] and not any(f in name or f in p for f in args[1:]):
            continue
        s, v, lead, n, pre = entry_chain(body)
        short = re.sub(r"\(.*$", "", p)
        print(f"{short[:64]:64s} swaits {s} vmwaits {v:2d} lead {lead:2d} loads {n:2d} preload {pre:2d}")


if __name__ == "__main__":
    main()
