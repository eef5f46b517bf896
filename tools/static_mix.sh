#!/bin/bash
# Static instruction mix of one kernel of the HIP library, without a GPU: cross-compiles the device
# code for gfx950 and prints, for every kernel whose demangled name contains PATTERN (fixed string),
# its code size, the compiler's kernel-resource-usage remarks and a count of every mnemonic.
#   bash tools/static_mix.sh 'epv_mh_propose2_kernel<true, true, 5>' [extra hipcc flags ...]
#   EPV_STATIC_MIX_KEEP=dir keeps the code object and the disassembly of each kernel in dir, and
#   reuses a code object already there (several kernels of one compile) WITHOUT looking at the
#   sources or the flags it was built from: one directory per source state and flag set.
set -euo pipefail
pat=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
llvm=$(dirname "$(realpath "$(command -v hipcc)")")/../lib/llvm/bin
[ -x "$llvm/llvm-objdump" ] || llvm=$(dirname "$(command -v llvm-objdump)")
tmp=${EPV_STATIC_MIX_KEEP:-$(mktemp -d)}
mkdir -p "$tmp"
[ -n "${EPV_STATIC_MIX_KEEP:-}" ] || trap 'rm -rf "$tmp"' EXIT
[ -s "$tmp/dev.co" ] ||
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -fvisibility=hidden \
  --cuda-device-only --no-gpu-bundle-output -c -fno-caret-diagnostics -Rpass-analysis=kernel-resource-usage "$@" \
  -I "$root/include" -I "$root/epievo_amd/csrc" -o "$tmp/dev.co" "$root/epievo_amd/csrc/epv_abi.hip" 2> "$tmp/remarks.txt"
# symbol table: value size type bind vis ndx name
"$llvm/llvm-readelf" -sW "$tmp/dev.co" | awk '$4 == "FUNC" { print $3, $8 }' | sort -u | while read -r size sym; do
  dem=$(c++filt "$sym")
  case "$dem" in *"$pat"*) ;; *) continue ;; esac
  echo "== $dem"
  echo "code size: $size bytes"
  grep -F "remark: " "$tmp/remarks.txt" | grep -F -A 12 "Function Name: $sym " | sed -e 's/^.*remark: //' -e 's/ \[-Rpass-analysis.*$//' | awk 'NR > 1 && /Function Name:/ { exit } { print }'
  "$llvm/llvm-objdump" -d --no-show-raw-insn --no-leading-addr --disassemble-symbols="$sym" "$tmp/dev.co" > "$tmp/$sym.s"
  echo "mnemonics:"
  awk '/^[ \t]+[a-z]/ { n[$1]++ } END { for (m in n) printf "%6d %s\n", n[m], m }' "$tmp/$sym.s" | sort -k1,1nr -k2
done
