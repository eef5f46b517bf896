// epv_patterns.h -- change patterns: what happened ACROSS the branches of the tree at one site of a sampled
// history.  A sample needs the 16-bit meta words alone (a = init state, k = number of jumps; no jump time is
// read) and the pre-order subtree[] array.  Per site, over the branches b (child node v = b + 1):
//   c = branches with k >= 1      K = sum of k
//   ng = branches with a == 0 and k odd (a net gain)      nl = branches with a == 1 and k odd (a net loss)
//   S_v = sum of k over the branches strictly below v (nodes v+1 .. v+subtree[v]-1), for every internal
//         non-root node v (subtree[v] > 1, v >= 1)
// A sample adds at most 1 to each of R = 12 + 2 B + I uint32 rows [R][cnt] (sites fastest; I = internal non-root
// nodes):
//   0..5 jumps_1..jumps_6   K == h           6 jumps_7plus     K >= 7            7 one_branch    c == 1
//   8 parallel_gain   ng >= 2                9 parallel_loss   nl >= 2           10 gain_and_loss ng >= 1 && nl >= 1
//   11 reverted_only  c >= 1 && ng == nl == 0
//   12 + b      sole_gain[b]   c == 1, the changed branch is b and nets a gain
//   12 + B + b  sole_loss[b]   the same for a net loss
//   12 + 2B + j clade_changed[j]   S_v >= 1, v the j-th internal non-root node in pre-order
// There is no dense row: a site without a jump anywhere on the tree stores nothing.  Every cell has one owner
// thread: plain loads and stores, no atomics.  An increment is at most 1 per sample: no cap below 2^32 samples.
#ifndef EPV_PATTERNS_H
#define EPV_PATTERNS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"

#define EPV_PAT_FIXED 12u   /* rows before the per-branch ones */
#define EPV_PAT_BCH 8u      /* branches whose meta loads are in flight together */

// one thread per site of lo .. lo + cnt - 1: sel once, then the current buffer's meta words of all branches in
// DESCENDING node order, EPV_PAT_BCH loads at a time (nothing is loaded below node 1).  nxt = the smallest
// changed node id seen so far, that is, among the nodes above the one the walk stands at: when the walk passes
// an internal node v (wave-uniform: subtree[v] is a scalar load), a changed node lies strictly below v iff
// nxt < v + subtree[v], because the nodes below v are the pre-order range v+1 .. v+subtree[v]-1.  The clade rows
// are numbered in pre-order, so the walk meets them from I - 1 down.  Any N, multifurcating and unary nodes
// included; no node masks, no LDS, no per-lane array.
__global__ __launch_bounds__(256) void epv_patterns_accum_kernel(EpvDev S, uint64_t lo, uint64_t cnt, uint32_t I,
                                                                 uint32_t *acc) {
  const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (s >= cnt) return;
  const uint64_t site = lo + s, n = S.n;
  const uint32_t B = S.B;
  const epv_meta_t *m = S.meta + (S.sel[site] ? (uint64_t)B * n : 0ull) + site;
  uint32_t *row = acc + s;
  uint32_t c = 0, K = 0, ng = 0, nl = 0, last = 0, nxt = 0xffffffffu;   // last: node << 2 | net change << 1 | loss
  uint32_t j = I;
  for (uint32_t v0 = B; v0 >= 1u; v0 = v0 > EPV_PAT_BCH ? v0 - EPV_PAT_BCH : 0u) {
    uint32_t w[EPV_PAT_BCH];
#pragma unroll
    for (uint32_t i = 0; i < EPV_PAT_BCH; ++i)   // nodes v0, v0 - 1, ...: branch v - 1
      w[i] = v0 > i ? (uint32_t)m[(uint64_t)(v0 - i - 1u) * n] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < EPV_PAT_BCH; ++i) {
      if (v0 <= i) break;
      const uint32_t v = v0 - i, sz = S.subtree[v];
      if (sz > 1u) {
        --j;
        if (nxt < v + sz) row[(uint64_t)(EPV_PAT_FIXED + 2u * B + j) * cnt] += 1u;
      }
      const uint32_t a = w[i] >> EPV_INIT_SHIFT, k = w[i] & EPV_NJ_MASK;
      if (!k) continue;
      ++c;
      K += k;
      if (k & 1u) { if (a) ++nl; else ++ng; }
      last = v << 2 | (k & 1u) << 1 | a;
      nxt = v;
    }
  }
  if (!c) return;
  row[(uint64_t)(K < 7u ? K - 1u : 6u) * cnt] += 1u;
  if (c == 1u) {
    row[7u * cnt] += 1u;
    if (last & 2u) row[(uint64_t)(EPV_PAT_FIXED + ((last & 1u) ? B : 0u) + (last >> 2) - 1u) * cnt] += 1u;
  }
  if (ng >= 2u) row[8u * cnt] += 1u;
  if (nl >= 2u) row[9u * cnt] += 1u;
  if (ng && nl) row[10u * cnt] += 1u;
  if (!(ng | nl)) row[11u * cnt] += 1u;
}

#endif
