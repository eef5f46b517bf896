// epv_turnover.h -- domain turnover: per branch, the runs of the state at its start (the parent's state as the
// branch sees it) and at its end (the child's state), each run KEPT (at least one of its sites has no net change
// on the branch) or TURNED OVER (every site of it changed): domains born and died, gaps filled and opened.  Joint
// along the genome like the domain size spectra (epv_domains.h), and joint across the two ends of a branch: a
// context counts a PART (include/epievo_mi355x.h, epv_set_domain_turnover), merged and closed on the host
// (host/epv_turnover.cpp).
//
// Rows of one sample, from the 16-bit meta word alone: X[2b] = a, X[2b + 1] = a XOR (k & 1) (a = init state,
// k = jumps of branch b at the site).  The keep word of a row and its partner r ^ 1 is K = ~(X ^ partner): a run
// is kept iff K has a bit inside it.
//
// Two launches per sample:
//   epv_rows_pack_kernel   the end rows (epv_rows.h) -> bits[r][tile]
//   epv_turn_runs_kernel   one block per chunk of EPV_DOM_CHUNK_WORDS words of one row: the runs kernel of the
//                          domain size spectra, with a pair (last end, OR of K after it) where that one carries
//                          the last end alone
// No block waits for another.  Integer adds commute and every edge record has one writer: the result depends on
// no launch shape.
#ifndef EPV_TURNOVER_H
#define EPV_TURNOVER_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"
#include "epv_domains.h"
#include "epv_rows.h"
#include "epv_turnover_rec.h"

// the keep word of word i of a row x and its partner y: bit j set where x and y agree and 64 i + j < cnt
__device__ __forceinline__ unsigned long long epv_turn_keep(unsigned long long x, unsigned long long y, uint64_t i,
                                                            uint64_t cnt) {
  unsigned long long k = ~(x ^ y);
  const uint64_t base = i * 64u;
  if (base + 64u > cnt) k &= base >= cnt ? 0ull : (~0ull >> (64u - (uint32_t)(cnt - base)));
  return k;
}

// what the scan carries: the last end so far as p + 1 (0 = none) and whether K has a bit after it
struct EpvTurnCarry {
  uint32_t last, tail;
};
// l lies before r
__device__ __forceinline__ EpvTurnCarry epv_turn_join(EpvTurnCarry l, EpvTurnCarry r) {
  if (r.last) return r;
  l.tail |= r.tail;
  return l;
}

// whether v holds for any of the block's 256 threads (every thread gets it); red: 4 words of LDS
__device__ __forceinline__ uint32_t epv_turn_block_any(bool v, uint32_t *red) {
  const unsigned long long b = __ballot(v);
  __syncthreads();   // (red may still be read from an earlier call)
  if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = b ? 1u : 0u;
  __syncthreads();
  return red[0] | red[1] | red[2] | red[3];
}

// grid (chunks, rows of this launch), 256 threads; row = r0 + blockIdx.y, partner = row ^ 1.  Positions are kept as
// p + 1 in 32 bits (0 = no end): cnt < 2^32.  hist [R][2][2][128] and len_sum [R][2][2] take the runs that end at
// an end and start after an earlier end; edge = this sample's records [R][2].
__global__ __launch_bounds__(256) void epv_turn_runs_kernel(const unsigned long long *bits, uint64_t words, uint64_t cnt,
                                                            uint32_t r0, unsigned long long *hist,
                                                            unsigned long long *len_sum, unsigned long long *edge) {
  __shared__ uint32_t table[4u * EPV_DOM_BINS];
  __shared__ uint32_t red[4];
  __shared__ uint32_t wave_last[4], wave_tail[4];
  __shared__ unsigned long long sums[4][4];
  const uint32_t t = threadIdx.x, r = r0 + blockIdx.y;
  const unsigned long long *row = bits + (uint64_t)r * words, *mate = bits + (uint64_t)(r ^ 1u) * words;
  const uint64_t c0 = (uint64_t)blockIdx.x * EPV_DOM_CHUNK_WORDS;   // the chunk's first word (< words)
  table[t] = 0u;
  table[t + 256u] = 0u;   // (2 x 2 x 128 = 512 cells)

  // this thread's words, their end masks and keep words; its last end and whether K has a bit after it
  const uint64_t i0 = c0 + (uint64_t)t * EPV_DOM_WPT;
  unsigned long long w[EPV_DOM_WPT + 1u], d[EPV_DOM_WPT], K[EPV_DOM_WPT];
#pragma unroll
  for (uint32_t j = 0; j <= EPV_DOM_WPT; ++j) w[j] = i0 + j < words ? row[i0 + j] : 0ull;
  EpvTurnCarry own = {0u, 0u};
#pragma unroll
  for (uint32_t j = 0; j < EPV_DOM_WPT; ++j) {
    const bool have = i0 + j < words;
    d[j] = have ? epv_dom_ends(w[j], w[j + 1u], i0 + j, cnt) : 0ull;
    K[j] = have ? epv_turn_keep(w[j], mate[i0 + j], i0 + j, cnt) : 0ull;
    if (d[j]) {
      const uint32_t b = 63u - (uint32_t)__builtin_clzll(d[j]);
      own.last = (uint32_t)((i0 + j) * 64u + b) + 1u;
      own.tail = b < 63u && (K[j] >> (b + 1u)) ? 1u : 0u;
    } else if (K[j]) {
      own.tail = 1u;
    }
  }

  // carry-in: the last end before the chunk and the OR of K after it up to the chunk, looked for 256 words at a
  // time towards the row's start.  A step without an end adds all its K to the tail
  EpvTurnCarry carry = {0u, 0u};
  for (uint64_t hi = c0; hi > 0u && carry.last == 0u;) {   // (block-uniform: carry comes from block reductions)
    const uint64_t lo_w = hi > 256u ? hi - 256u : 0u, i = lo_w + t;
    uint32_t e = 0u;
    bool after = false;   // K has a bit in this word after the word's last end
    if (i < hi) {
      const unsigned long long x = row[i];
      const unsigned long long dd = epv_dom_ends(x, row[i + 1u], i, cnt);   // (i + 1 <= c0 < words)
      const unsigned long long kk = epv_turn_keep(x, mate[i], i, cnt);
      if (dd) {
        const uint32_t b = 63u - (uint32_t)__builtin_clzll(dd);
        e = (uint32_t)(i * 64u + b) + 1u;
        after = b < 63u && (kk >> (b + 1u));
      } else {
        after = kk != 0ull;
      }
    }
    const uint32_t m = epv_dom_block_max(e, red);
    // the words that lie after the end m: the word that holds it, and the words without an end behind it
    const bool counts = i < hi && (m == 0u || e == m || (e == 0u && i * 64u >= (uint64_t)m));
    carry.tail |= epv_turn_block_any(counts && after, red);
    carry.last = m;
    hi = lo_w;
  }

  // inclusive scan of the pairs over the block: shuffles inside a wave, LDS across the four waves
  EpvTurnCarry inc = own;
  const uint32_t lane = t & 63u, wave = t >> 6;
  for (int s = 1; s < 64; s <<= 1) {
    EpvTurnCarry o;
    o.last = (uint32_t)__shfl_up((int)inc.last, (unsigned)s, 64);
    o.tail = (uint32_t)__shfl_up((int)inc.tail, (unsigned)s, 64);
    if (lane >= (uint32_t)s) inc = epv_turn_join(o, inc);
  }
  EpvTurnCarry prev;   // exclusive, within the wave
  prev.last = (uint32_t)__shfl_up((int)inc.last, 1u, 64);
  prev.tail = (uint32_t)__shfl_up((int)inc.tail, 1u, 64);
  if (lane == 0u) prev.last = prev.tail = 0u;
  if (lane == 63u) { wave_last[wave] = inc.last; wave_tail[wave] = inc.tail; }
  __syncthreads();   // (also: table is zeroed)
  EpvTurnCarry before = carry;
  for (uint32_t x = 0; x < wave; ++x) before = epv_turn_join(before, EpvTurnCarry{wave_last[x], wave_tail[x]});
  prev = epv_turn_join(before, prev);

  // walk the ends lowest first: length = p + 1 - prev, state = bit p, kept = K has a bit since the previous end
  unsigned long long sum[4] = {0ull, 0ull, 0ull, 0ull};
  uint32_t at = prev.last, acc = prev.tail;
#pragma unroll
  for (uint32_t j = 0; j < EPV_DOM_WPT; ++j) {
    unsigned long long dd = d[j];
    const uint32_t base = (uint32_t)((i0 + j) * 64u);
    uint32_t from = 0u;   // the first bit of this word that belongs to the open run
    while (dd) {
      const uint32_t b = (uint32_t)__ffsll((long long)dd) - 1u;
      dd &= dd - 1ull;
      const unsigned long long in_run = (~0ull << from) & (~0ull >> (63u - b));   // (from <= b)
      const uint32_t kept = (acc || (K[j] & in_run)) ? 1u : 0u;
      const uint32_t p1 = base + b + 1u, st = (uint32_t)(w[j] >> b) & 1u, len = p1 - at;
      if (at == 0u) {   // the row's first end: the run from the stretch's first site, which only a merge can close
        edge[(uint64_t)r * 2u] = (unsigned long long)len | ((unsigned long long)kept << EPV_TURN_KEPT_SHIFT) |
                                 ((unsigned long long)st << EPV_DOM_STATE_SHIFT);
      } else {
        const uint32_t cls = st * 2u + kept;
        atomicAdd(&table[cls * EPV_DOM_BINS + epv_domain_bin(len)], 1u);
#pragma unroll
        for (uint32_t q = 0; q < 4u; ++q) sum[q] += q == cls ? len : 0u;
      }
      at = p1;
      acc = 0u;
      from = b + 1u;
    }
    if (from < 64u && (K[j] >> from)) acc = 1u;
  }

  // the row's last word is in this block: the run from the last end to the last site, or the whole stretch
  if (c0 + EPV_DOM_CHUNK_WORDS >= words) {
    if (t == 0u) {
      EpvTurnCarry all = carry;
      for (uint32_t x = 0; x < 4u; ++x) all = epv_turn_join(all, EpvTurnCarry{wave_last[x], wave_tail[x]});
      const unsigned long long st = (row[(cnt - 1u) >> 6] >> ((cnt - 1u) & 63u)) & 1ull;
      const unsigned long long flags = (st << EPV_DOM_STATE_SHIFT) | ((unsigned long long)all.tail << EPV_TURN_KEPT_SHIFT);
      if (all.last == 0u) {
        edge[(uint64_t)r * 2u] = cnt | EPV_DOM_WHOLE | flags;
        edge[(uint64_t)r * 2u + 1u] = cnt | EPV_DOM_WHOLE | flags;
      } else {
        edge[(uint64_t)r * 2u + 1u] = (cnt - all.last) | flags;
      }
    }
  }

  // flush: the nonzero cells, and the length sums after a block reduction
  for (int s = 1; s < 64; s <<= 1) {
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) sum[q] += __shfl_xor(sum[q], s, 64);
  }
  if (lane == 0u) {
#pragma unroll
    for (uint32_t q = 0; q < 4u; ++q) sums[q][wave] = sum[q];
  }
  __syncthreads();   // (table complete as well)
#pragma unroll
  for (uint32_t h = 0; h < 2u; ++h) {
    const uint32_t cell = table[t + 256u * h];
    if (cell) atomicAdd(hist + (uint64_t)r * 4u * EPV_DOM_BINS + t + 256u * h, (unsigned long long)cell);
  }
  if (t < 4u) {
    const unsigned long long total = sums[t][0] + sums[t][1] + sums[t][2] + sums[t][3];
    if (total) atomicAdd(len_sum + (uint64_t)r * 4u + t, total);
  }
}

#endif
