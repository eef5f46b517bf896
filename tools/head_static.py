#!/usr/bin/env python3
"""The head of the fused colour phase in the compiled kernel, without a GPU: for every fused body
epv_mh_propose2_kernel<true, true, NN> in a directory made by tools/static_mix.sh with EPV_STATIC_MIX_KEEP
(run it with the pattern 'epv_mh_propose2_kernel<true, true' first), the instructions between the kernel's
entry and its first wave scan (the first DPP instruction: wave_incl_scan_u32 of the planning round):
  global loads, s_waitcnt with a vmcnt, s_cbranch, and
  loads in a loop       global loads between a backward branch in the region and its target
  sel before wait       bytes of S.sel (byte and short loads ahead of the barrier) issued before the first vmcnt wait
  waits inside batch 2  vmcnt waits between the first and the last 16-bit load behind the barrier (meta + outer columns)
    python tools/head_static.py DIR [DIR ...]"""
import glob
import os
import re
import sys


def head(path):
    """-> [(address, mnemonic, text)] up to the first DPP instruction, and the address of the symbol"""
    ins, base = [], None
    for line in open(path):
        m = re.match(r"\s+([a-z_0-9]+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):(.*)$", line)
        if not m:
            continue
        addr = int(m.group(3), 16)
        base = addr if base is None else base
        if "dpp" in line or "row_shr" in line:
            break
        ins.append((addr, m.group(1), m.group(2), m.group(4)))      # (a branch's target stands behind the encoding)
    return ins, base


def vm_wait(mn, ops):
    return mn == "s_waitcnt" and "vmcnt" in ops


def analyse(path):
    ins, base = head(path)
    loads = [i for i, x in enumerate(ins) if x[1].startswith("global_load")]
    waits = [i for i, x in enumerate(ins) if vm_wait(x[1], x[2])]
    barrier = next((i for i, x in enumerate(ins) if x[1] == "s_barrier"), len(ins))
    in_loop = set()
    for i, (addr, mn, ops, tail) in enumerate(ins):
        m = re.search(r"<[^>]*\+0x([0-9a-f]+)>", tail) if mn.startswith("s_cbranch") or mn == "s_branch" else None
        if m and base + int(m.group(1), 16) <= addr:
            target = base + int(m.group(1), 16)
            in_loop.update(j for j in loads if target <= ins[j][0] <= addr)
    first_wait = waits[0] if waits else len(ins)
    width = {"global_load_ubyte": 1, "global_load_sbyte": 1, "global_load_ushort": 2, "global_load_sshort": 2}
    sel = sum(width.get(ins[j][1], 0) for j in loads if j < barrier and j < first_wait)
    batch2 = [j for j in loads if j > barrier and ins[j][1] == "global_load_ushort"]
    inside = [w for w in waits if batch2 and batch2[0] < w < batch2[-1]]
    return dict(instructions=len(ins), loads=len(loads), waits=len(waits),
                branches=sum(1 for x in ins if x[1].startswith("s_cbranch")), in_loop=len(in_loop), sel=sel,
                batch2=len(batch2), inside=len(inside))


for d in sys.argv[1:]:
    print("== %s" % d)
    print("  NN  instructions  global loads  vmcnt waits  s_cbranch  loads in a loop  sel bytes before the first wait"
          "  16-bit loads behind the barrier / vmcnt waits among them")
    for nn in (5, 4, 3, 2, 0):
        f = glob.glob(os.path.join(d, "_Z22epv_mh_propose2_kernelILb1ELb1ELi%dEE*.s" % nn))
        if not f:
            print("  %d   (no disassembly: run tools/static_mix.sh with EPV_STATIC_MIX_KEEP=%s first)" % (nn, d))
            continue
        r = analyse(f[0])
        print("  %d   %12d  %12d  %11d  %9d  %15d  %31d  %10d / %d" % (nn, r["instructions"], r["loads"], r["waits"],
              r["branches"], r["in_loop"], r["sel"], r["batch2"], r["inside"]))
