#!/usr/bin/env python3
"""Which kernels of the HIP library did a change touch, and what do the new ones cost?  Without a GPU.

  python tools/kernel_streams.py DIR_BEFORE DIR_AFTER [NEW_PATTERN]

DIR_*: directories made by tools/static_mix.sh with EPV_STATIC_MIX_KEEP=dir, one per source state (dev.co, the gfx950
code object, and remarks.txt, the compiler's kernel-resource-usage remarks).  Every kernel is disassembled
(llvm-objdump -d per symbol; addresses and address comments left out) and compared by its DEMANGLED name, so an
instantiation that only gained an empty trailing template pack is compared with its former self.  One line per kernel:
same | CHANGED | NEW, with VGPRs, AGPRs, SGPR spills, VGPR spills, scratch, LDS and waves per SIMD of the state after.
"""
import os
import re
import shutil
import subprocess
import sys


def llvm_bin():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    d = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "lib", "llvm", "bin")
    return d if os.path.exists(os.path.join(d, "llvm-objdump")) else os.path.dirname(shutil.which("llvm-objdump"))


def kernels(d):
    """demangled name (arguments cut) -> mangled symbol"""
    out = subprocess.run([os.path.join(llvm_bin(), "llvm-readelf"), "-sW", os.path.join(d, "dev.co")],
                         check=True, capture_output=True, text=True).stdout
    syms = sorted({f[7] for f in (l.split() for l in out.splitlines()) if len(f) >= 8 and f[3] == "FUNC"})
    dem = subprocess.run(["c++filt"], input="\n".join(syms), check=True, capture_output=True, text=True).stdout.splitlines()
    return {re.sub(r"\(.*$", "", n): s for n, s in zip(dem, syms)}


def stream(d, sym):
    out = subprocess.run([os.path.join(llvm_bin(), "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                          "--disassemble-symbols=" + sym, os.path.join(d, "dev.co")],
                         check=True, capture_output=True, text=True).stdout
    ins = [re.sub(r"\s*<[^>]*>$", "", re.sub(r"\s*//.*$", "", l)) for l in out.splitlines() if re.match(r"^[ \t]+[a-z]", l)]
    while ins and re.match(r"^\s*(s_nop 0|s_code_end)\s*$", ins[-1]):     # padding behind the last kernel
        ins.pop()
    return ins


def resources(d):
    """mangled symbol -> the figures of the compiler's remarks"""
    res, cur = {}, None
    keys = (("VGPRs", r" VGPRs: (\d+)"), ("AGPRs", r"AGPRs: (\d+)"), ("SGPRspill", r"SGPRs Spill: (\d+)"),
            ("VGPRspill", r"VGPRs Spill: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
            ("LDS", r"LDS Size \[bytes/block\]: (\d+)"), ("waves", r"Occupancy \[waves/SIMD\]: (\d+)"))
    for l in open(os.path.join(d, "remarks.txt"), errors="replace"):
        m = re.search(r"Function Name: (\S+)", l)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        if cur is None:
            continue
        for k, pat in keys:
            m = re.search(pat, l)
            if m and k not in cur:
                cur[k] = int(m.group(1))
    return res


def main():
    a, b = sys.argv[1], sys.argv[2]
    ka, kb, rb = kernels(a), kernels(b), resources(b)
    same = changed = new = 0
    print("kernel | VGPRs AGPRs SGPR-spill VGPR-spill scratch[bytes/lane] LDS[bytes/block] occupancy[waves/SIMD]")
    for name in sorted(set(ka) | set(kb), key=lambda n: (len(n), n)):
        if name not in kb:
            print("MISSING %s" % name)
            continue
        r = rb.get(kb[name], {})
        fig = " ".join(str(r.get(k, "?")) for k in ("VGPRs", "AGPRs", "SGPRspill", "VGPRspill", "scratch", "LDS", "waves"))
        if name not in ka:
            new += 1
            print("NEW     %s | %s" % (name, fig))
            continue
        sa, sb = stream(a, ka[name]), stream(b, kb[name])
        if sa == sb:
            same += 1
            print("same    %s | %s  (%d instructions)" % (name, fig, len(sb)))
        else:
            changed += 1
            print("CHANGED %s | %s  (%d -> %d instructions)" % (name, fig, len(sa), len(sb)))
    print("kernels before: %d after: %d same: %d changed: %d new: %d missing: %d"
          % (len(ka), len(kb), same, changed, new, len(set(ka) - set(kb))))
    return 1 if changed or set(ka) - set(kb) else 0


if __name__ == "__main__":
    sys.exit(main())
