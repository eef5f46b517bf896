#!/bin/bash
# Which kernels of the HIP library did a change touch?  Without a GPU: disassembles every kernel of two
# device code objects (made by tools/static_mix.sh with EPV_STATIC_MIX_KEEP=dir, one directory per source
# state) and compares them instruction for instruction (operands included, addresses left out).
#   bash tools/static_diff.sh DIR_BEFORE DIR_AFTER
# prints one line per kernel: same | CHANGED (instructions before -> after) | only in one of the two.
set -euo pipefail
a=$1; b=$2
llvm=$(dirname "$(realpath "$(command -v hipcc)")")/../lib/llvm/bin
[ -x "$llvm/llvm-objdump" ] || llvm=$(dirname "$(command -v llvm-objdump)")
syms() { "$llvm/llvm-readelf" -sW "$1/dev.co" | awk '$4 == "FUNC" { print $8 }' | sort -u; }
dis() {  # directory, symbol -> instructions only
  "$llvm/llvm-objdump" -d --no-show-raw-insn --no-leading-addr --disassemble-symbols="$2" "$1/dev.co" |
    awk '/^[ \t]+[a-z]/' | sed -e 's#[ \t]*//.*$##' -e 's/[ \t]*<[^>]*>$//' |
    awk '{ l[NR] = $0 } END { n = NR; while (n > 0 && l[n] ~ /^[ \t]*(s_nop 0|s_code_end)[ \t]*$/) n--;   # (padding behind the last kernel)
                             for (i = 1; i <= n; i++) print l[i] }'
}
same=0; changed=0
for sym in $( (syms "$a"; syms "$b") | sort -u ); do
  dem=$(c++filt "$sym" | sed -e 's/(.*$//')
  ina=$(syms "$a" | grep -cxF "$sym" || true); inb=$(syms "$b" | grep -cxF "$sym" || true)
  if [ "$ina" = 0 ]; then echo "only after   $dem"; continue; fi
  if [ "$inb" = 0 ]; then echo "only before  $dem"; continue; fi
  dis "$a" "$sym" > "$a/cmp_a.txt"; dis "$b" "$sym" > "$b/cmp_b.txt"
  if cmp -s "$a/cmp_a.txt" "$b/cmp_b.txt"; then
    same=$((same + 1)); echo "same         $dem ($(wc -l < "$a/cmp_a.txt") instructions)"
  else
    changed=$((changed + 1)); echo "CHANGED      $dem ($(wc -l < "$a/cmp_a.txt") -> $(wc -l < "$b/cmp_b.txt") instructions)"
  fi
done
echo "$same kernels identical, $changed changed"
