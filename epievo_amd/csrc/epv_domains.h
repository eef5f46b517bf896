// epv_domains.h -- domain size spectra: the run lengths of every node's state along the genome, counted over
// the sampled histories.  The first accumulator that is joint along the genome: a run can cross any tile,
// block, context or GPU boundary, so a context counts a PART (include/epievo_mi355x.h, epv_set_domain_stats):
// the runs closed inside its stretch of sites in hist / len_sum, and per sample and node the two runs the
// stretch cannot close as edge records.  Parts are merged and closed on the host (host/epv_domains.cpp).
//
// Node states of one sample, from the 16-bit meta word alone (no jump time is read): x_v[s] = a XOR (k & 1)
// for a node v >= 1 (a = init state, k = jumps of branch v at site s); x_0[s] = a of the branch of the root's
// lowest-numbered child.  Over a stretch of cnt sites an END is a position p with p + 1 < cnt and
// x[p] != x[p + 1]; the run that ends there has length p - p' (p' = the previous end) and state x[p].
//
// Two launches per sample:
//   epv_rows_pack_kernel  the node rows of state 1 (epv_rows.h) -> bits[v][tile] (64-bit words)
//   epv_dom_runs_kernel   one block per chunk of EPV_DOM_CHUNK_WORDS words of one node's row: end masks, the
//                         position of the last end before each thread's words (a cooperative look-back for the
//                         chunk, a prefix maximum inside it), run lengths binned in LDS
// No block waits for another: a block that needs the last end before its chunk reads the bit words before it.
// Integer adds commute and every edge record has one writer: the result depends on no launch shape.
#ifndef EPV_DOMAINS_H
#define EPV_DOMAINS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"
#include "epv_domain_bin.h"
#include "epv_rows.h"

#define EPV_DOM_CHUNK_WORDS 1024u     /* words of a node's row per block of the runs kernel: 65 536 sites */
#define EPV_DOM_WPT (EPV_DOM_CHUNK_WORDS / 256u)   /* consecutive words per thread */

// the end mask of word i of a row: bit j set where x[64 i + j] != x[64 i + j + 1] and 64 i + j + 1 < cnt
__device__ __forceinline__ unsigned long long epv_dom_ends(unsigned long long w, unsigned long long next, uint64_t i,
                                                           uint64_t cnt) {
  unsigned long long d = w ^ ((w >> 1) | (next << 63));
  const uint64_t base = i * 64u;   // positions below cnt - 1 stay
  if (base + 64u > cnt - 1u) d &= base >= cnt - 1u ? 0ull : (~0ull >> (64u - (uint32_t)(cnt - 1u - base)));
  return d;
}

// the maximum of v over the block's 256 threads (every thread gets it); red: 4 words of LDS
__device__ __forceinline__ uint32_t epv_dom_block_max(uint32_t v, uint32_t *red) {
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)v, d, 64);
    v = o > v ? o : v;
  }
  __syncthreads();   // (red may still be read from an earlier call)
  if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const uint32_t a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
  return a > b ? a : b;
}

// grid (chunks, nodes of this launch), 256 threads; row = v0 + blockIdx.y.  Positions are kept as p + 1 in 32
// bits (0 = no end): cnt < 2^32.  hist [N][2][128] and len_sum [N][2] take the runs that end at an end and start
// after an earlier end; edge = this sample's records [N][2].
__global__ __launch_bounds__(256) void epv_dom_runs_kernel(const unsigned long long *bits, uint64_t words, uint64_t cnt,
                                                           uint32_t v0, unsigned long long *hist,
                                                           unsigned long long *len_sum, unsigned long long *edge) {
  __shared__ uint32_t table[2u * EPV_DOM_BINS];
  __shared__ uint32_t red[4];
  __shared__ uint32_t wave_last[4];
  __shared__ unsigned long long sums[2][4];
  const uint32_t t = threadIdx.x, v = v0 + blockIdx.y;
  const unsigned long long *row = bits + (uint64_t)v * words;
  const uint64_t c0 = (uint64_t)blockIdx.x * EPV_DOM_CHUNK_WORDS;   // the chunk's first word (< words)
  table[t] = 0u;   // (2 x 128 = 256 cells)

  // this thread's words and their end masks
  const uint64_t i0 = c0 + (uint64_t)t * EPV_DOM_WPT;
  unsigned long long w[EPV_DOM_WPT + 1u], d[EPV_DOM_WPT];
#pragma unroll
  for (uint32_t j = 0; j <= EPV_DOM_WPT; ++j) w[j] = i0 + j < words ? row[i0 + j] : 0ull;
  uint32_t last = 0u;   // this thread's last end, as p + 1
#pragma unroll
  for (uint32_t j = 0; j < EPV_DOM_WPT; ++j) {
    d[j] = i0 + j < words ? epv_dom_ends(w[j], w[j + 1u], i0 + j, cnt) : 0ull;
    if (d[j]) last = (uint32_t)((i0 + j) * 64u + (63u - (uint32_t)__builtin_clzll(d[j]))) + 1u;
  }

  // carry-in: the last end before the chunk, looked for 256 words at a time towards the row's start
  uint32_t carry = 0u;
  for (uint64_t hi = c0; hi > 0u && carry == 0u;) {   // (block-uniform: carry comes from epv_dom_block_max)
    const uint64_t lo_w = hi > 256u ? hi - 256u : 0u, i = lo_w + t;
    uint32_t e = 0u;
    if (i < hi) {
      const unsigned long long dd = epv_dom_ends(row[i], row[i + 1u], i, cnt);   // (i + 1 <= c0 < words)
      if (dd) e = (uint32_t)(i * 64u + (63u - (uint32_t)__builtin_clzll(dd))) + 1u;
    }
    carry = epv_dom_block_max(e, red);
    hi = lo_w;
  }

  // inclusive prefix maximum of `last` over the block: shuffles inside a wave, LDS across the four waves
  uint32_t inc = last;
  const uint32_t lane = t & 63u, wave = t >> 6;
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)inc, (unsigned)s, 64);
    if (lane >= (uint32_t)s && o > inc) inc = o;
  }
  uint32_t prev = (uint32_t)__shfl_up((int)inc, 1u, 64);   // exclusive, within the wave
  if (lane == 0u) prev = 0u;
  if (lane == 63u) wave_last[wave] = inc;
  __syncthreads();   // (also: table is zeroed)
  uint32_t before = carry;
  for (uint32_t x = 0; x < wave; ++x) before = wave_last[x] > before ? wave_last[x] : before;
  prev = prev > before ? prev : before;

  // walk the ends lowest first: length = p + 1 - prev, state = bit p
  unsigned long long sum0 = 0ull, sum1 = 0ull;
#pragma unroll
  for (uint32_t j = 0; j < EPV_DOM_WPT; ++j) {
    unsigned long long dd = d[j];
    const uint32_t base = (uint32_t)((i0 + j) * 64u);
    while (dd) {
      const uint32_t b = (uint32_t)__ffsll((long long)dd) - 1u;
      dd &= dd - 1ull;
      const uint32_t p1 = base + b + 1u, st = (uint32_t)(w[j] >> b) & 1u, len = p1 - prev;
      if (prev == 0u) {   // the row's first end: the run from the stretch's first site, which only a merge can close
        edge[(uint64_t)v * 2u] = (unsigned long long)len | ((unsigned long long)st << EPV_DOM_STATE_SHIFT);
      } else {
        atomicAdd(&table[st * EPV_DOM_BINS + epv_domain_bin(len)], 1u);
        if (st) sum1 += len; else sum0 += len;
      }
      prev = p1;
    }
  }

  // the row's last word is in this block: the run from the last end to the last site, or the whole stretch
  if (c0 + EPV_DOM_CHUNK_WORDS >= words) {
    uint32_t all = wave_last[0];
    for (uint32_t x = 1; x < 4u; ++x) all = wave_last[x] > all ? wave_last[x] : all;
    all = all > carry ? all : carry;
    if (t == 0u) {
      const unsigned long long st = (row[(cnt - 1u) >> 6] >> ((cnt - 1u) & 63u)) & 1ull;
      if (all == 0u) {
        const unsigned long long rec = cnt | EPV_DOM_WHOLE | (st << EPV_DOM_STATE_SHIFT);
        edge[(uint64_t)v * 2u] = rec;
        edge[(uint64_t)v * 2u + 1u] = rec;
      } else {
        edge[(uint64_t)v * 2u + 1u] = (cnt - all) | (st << EPV_DOM_STATE_SHIFT);
      }
    }
  }

  // flush: the nonzero cells, and the length sums after a block reduction
  for (int s = 1; s < 64; s <<= 1) {
    sum0 += __shfl_xor(sum0, s, 64);
    sum1 += __shfl_xor(sum1, s, 64);
  }
  if (lane == 0u) { sums[0][wave] = sum0; sums[1][wave] = sum1; }
  __syncthreads();   // (table complete as well)
  const uint32_t cell = table[t];
  if (cell) atomicAdd(hist + (uint64_t)v * 2u * EPV_DOM_BINS + t, (unsigned long long)cell);
  if (t < 2u) {
    const unsigned long long total = sums[t][0] + sums[t][1] + sums[t][2] + sums[t][3];
    if (total) atomicAdd(len_sum + (uint64_t)v * 2u + t, total);
  }
}

#endif
