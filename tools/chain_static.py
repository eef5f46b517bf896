#!/usr/bin/env python3
"""The fused colour phase section by section in the compiled kernel, without a GPU (sibling of tools/head_static.py).
For a directory made by tools/static_mix.sh with EPV_STATIC_MIX_KEEP and -DEPV_P2_PROFILE (pattern
'epv_mh_propose2_kernel<true, true'), the disassembly of a fused body is cut at its s_memtime instructions -- the
kernel's entry and P2_MARK(0) .. P2_MARK(9) (and P2_MARK(10) behind pruning), in the order the compiler laid the code out, which is the order of the
source here -- and for every section of the body the tool counts
  instructions, global loads (16-bit ones, byte ones), vmcnt waits (full ones: vmcnt(0)), lgkmcnt waits, LDS instructions
and, from the compiler's remarks, prints VGPRs, scratch, occupancy and spilled SGPRs of all fused bodies.
    python tools/chain_static.py [--nn 5] DIR [DIR ...]"""
import glob
import os
import re
import sys

SECTIONS = ["head", "scan/plan", "descriptor pass", "dense eval", "pruning", "downward", "hand-over", "search",
            "assembly", "acceptance"]
# ... with the dense evaluation in two passes (8-double records): P2_MARK(10) sits behind pruning
SECTIONS2 = SECTIONS[:5] + ["dense eval 2"] + SECTIONS[5:]


def instructions(path):
    out = []
    for line in open(path):
        m = re.match(r"\s+([a-z_0-9]+)\s*(.*?)\s*//\s*[0-9A-Fa-f]+:", line)
        if m:
            out.append((m.group(1), m.group(2)))
    return out


def sections(ins):
    cuts = [i for i, x in enumerate(ins) if x[0] == "s_memtime"]
    return [ins[a + 1:b] for a, b in zip(cuts[:-1], cuts[1:])]


def count(sec):
    vm = [ops for mn, ops in sec if mn == "s_waitcnt" and "vmcnt" in ops]
    return dict(n=len(sec),
                gl=sum(1 for mn, _ in sec if mn.startswith("global_load")),
                gl16=sum(1 for mn, _ in sec if mn.startswith(("global_load_ushort", "global_load_short_d16"))),
                gl8=sum(1 for mn, _ in sec if mn.startswith(("global_load_ubyte", "global_load_sbyte"))),
                gs=sum(1 for mn, _ in sec if mn.startswith("global_store")),
                vm=len(vm), vm0=sum(1 for ops in vm if "vmcnt(0)" in ops),
                lgkm=sum(1 for mn, ops in sec if mn == "s_waitcnt" and "lgkmcnt" in ops),
                lds=sum(1 for mn, _ in sec if mn.startswith("ds_")))


def resources(d):
    """{NN: (VGPRs, scratch, occupancy, spilled SGPRs)} from remarks.txt"""
    out, nn = {}, None
    for line in open(os.path.join(d, "remarks.txt")):
        m = re.search(r"Function Name: _Z22epv_mh_propose2_kernelILb1ELb1ELi(\d)E(?:Lb0EJE)?E", line)
        if "Function Name:" in line:
            nn = int(m.group(1)) if m else None
            if nn is not None:
                out[nn] = {}
            continue
        if nn is None:
            continue
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("sspill", r"SGPRs Spill: (\d+)")):
            m = re.search(pat, line)
            if m:
                out[nn][key] = int(m.group(1))
    return out


args = sys.argv[1:]
nn = 5
if args and args[0] == "--nn":
    nn, args = int(args[1]), args[2:]
for d in args:
    print("== %s, NN = %d" % (d, nn))
    # (the default body: not the direct one, no leaf arguments)
    f = (glob.glob(os.path.join(d, "_Z22epv_mh_propose2_kernelILb1ELb1ELi%dELb0EJEE*.s" % nn)) or
         glob.glob(os.path.join(d, "_Z22epv_mh_propose2_kernelILb1ELb1ELi%dEE*.s" % nn)))
    if not f:
        print("  (no disassembly: run tools/static_mix.sh with EPV_STATIC_MIX_KEEP=%s -DEPV_P2_PROFILE first)" % d)
        continue
    secs = sections(instructions(f[0]))
    names = SECTIONS2 if len(secs) == len(SECTIONS2) else SECTIONS
    if len(secs) != len(names):
        print("  (%d sections, expected %d: not a -DEPV_P2_PROFILE build; registers only)" % (len(secs), len(SECTIONS2)))
        secs = []
    else:
        print("  %-16s %12s %12s %8s %7s %13s %18s %13s %5s" % ("section", "instructions", "global loads", "16-bit", "byte",
                                                              "global stores", "vmcnt waits / (0)", "lgkmcnt waits", "LDS"))
    for name, sec in zip(names, secs):
        c = count(sec)
        print("  %-16s %12d %12d %8d %7d %13d %12d / %-3d %13d %5d" % (name, c["n"], c["gl"], c["gl16"], c["gl8"], c["gs"],
                                                                       c["vm"], c["vm0"], c["lgkm"], c["lds"]))
    res = resources(d)
    for k in sorted(res, reverse=True):
        r = res[k]
        print("  NN = %d: %d VGPRs, scratch %d B, %d waves per SIMD, %d spilled SGPRs" % (k, r.get("vgpr", -1), r.get("scratch", -1),
                                                                                        r.get("occ", -1), r.get("sspill", -1)))
