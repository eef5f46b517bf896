// epv_rows.h -- the bit rows of one sample: what the five summaries that are joint along the genome (epv_domains.h,
// epv_turnover.h, epv_corr.h, epv_dmaps.h, epv_tracts.h) count from.  One kernel packs the counted sites of the
// resident paths into rows of 64-bit words, 64 consecutive sites a word, from the 16-bit meta word alone (no jump
// time is read): a = the init state of branch b at the site, k = its jumps, y = a XOR (k & 1) its end state.
//
//   EPV_ROWS_NODE     N rows      bits[v] = (x_v == state), x_v = y of branch v for a node v >= 1, x_0 = a of the
//                                 branch of the root's lowest-numbered child (child0)
//   EPV_ROWS_CORR     N + B rows  the node rows, then bits[N + b] = k & 1, the net change of branch b
//   EPV_ROWS_ENDS     2 B rows    bits[2b] = a, bits[2b + 1] = y: the two ends of branch b
//
// bits[r * words + tile]: bit j of a word = row r at site lo + 64 tile + j, zero beyond cnt.  Tiles start at lo, not
// at a multiple of 64.  Each layer packs into its own scratch and counts from it with its own kernel.
#ifndef EPV_ROWS_H
#define EPV_ROWS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"

#define EPV_DOM_BCH 8u                /* branches whose meta loads are in flight together */

enum EpvRows : uint32_t { EPV_ROWS_NODE, EPV_ROWS_CORR, EPV_ROWS_ENDS };

// One wave per tile of 64 consecutive counted sites; blockDim = 256: four tiles per block, (words + 3) / 4 blocks.
// sel once, then the current buffer's meta words of all branches, EPV_DOM_BCH loads at a time.  child0 and state
// are read by the node rows alone.
template <uint32_t ROWS>
__global__ __launch_bounds__(256) void epv_rows_pack_kernel(EpvDev S, uint64_t lo, uint64_t cnt, uint64_t words,
                                                            uint32_t child0, uint32_t state, unsigned long long *bits) {
  const uint64_t tile = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (tile >= words) return;   // (wave-uniform, and ahead of every ballot)
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t s = tile * 64u + lane, n = S.n;
  const bool in = s < cnt;
  const uint64_t site = lo + (in ? s : cnt - 1u);   // (a lane beyond the range reads the last site and counts as 0)
  const uint32_t B = S.B, N = S.N;
  const epv_meta_t *m = S.meta + (S.sel[site] ? (uint64_t)B * n : 0ull) + site;
  for (uint32_t b0 = 0; b0 < B; b0 += EPV_DOM_BCH) {
    uint32_t w[EPV_DOM_BCH];
#pragma unroll
    for (uint32_t i = 0; i < EPV_DOM_BCH; ++i) w[i] = b0 + i < B ? (uint32_t)m[(uint64_t)(b0 + i) * n] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < EPV_DOM_BCH; ++i) {
      if (b0 + i >= B) break;   // (uniform)
      const uint32_t b = b0 + i, a = (w[i] >> EPV_INIT_SHIFT) & 1u, k = w[i] & EPV_NJ_MASK, y = (a ^ k) & 1u;
      if (ROWS == EPV_ROWS_ENDS) {
        const unsigned long long xa = __ballot(in && a);
        const unsigned long long xe = __ballot(in && y);
        if (lane == 0u) {
          bits[(uint64_t)(2u * b) * words + tile] = xa;
          bits[(uint64_t)(2u * b + 1u) * words + tile] = xe;
        }
      } else {
        const unsigned long long x = __ballot(in && y == state);
        const unsigned long long r = __ballot(in && a == state);
        const unsigned long long ch = ROWS == EPV_ROWS_CORR ? __ballot(in && (k & 1u)) : 0ull;
        if (lane == 0u) {
          bits[(uint64_t)(b + 1u) * words + tile] = x;
          if (b + 1u == child0) bits[tile] = r;
          if (ROWS == EPV_ROWS_CORR) bits[(uint64_t)(N + b) * words + tile] = ch;
        }
      }
    }
  }
}

#endif
