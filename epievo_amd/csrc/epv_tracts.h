// epv_tracts.h -- change tracts: per branch, the maximal runs of sites with a net change, each classified by its
// direction (all gained, all lost, mixed) and by the state of the unchanged site on each flank, its length binned
// like the domain size spectra.  A gained tract between flanks 0 and 0 is a domain born, with flanks 0 | 1 a
// domain that grew by that many sites at its left edge, with flanks 1 | 1 a gap filled; lost tracts likewise.
// Joint along the genome and across the two ends of a branch, like the domain turnover (epv_turnover.h): a context
// counts a PART (include/epievo_mi355x.h, epv_set_change_tracts), merged and closed on the host
// (host/epv_tracts.cpp).
//
// Rows of one sample are the turnover's: bits[2b] = a, bits[2b + 1] = y = a XOR (k & 1).  C = a ^ y is the net
// change.  A tract STARTS at p where C[p] = 1 and C[p - 1] = 0 (or p = 0) and ENDS at p where C[p] = 1, C[p + 1] = 0
// and p + 1 < cnt; a tract that holds the stretch's first or last site goes to an edge record (epv_tract_rec.h).
//
// Two launches per sample:
//   epv_rows_pack_kernel    the end rows (epv_rows.h), as the turnover packs them, into this layer's own scratch
//   epv_tract_runs_kernel   one block per chunk of EPV_DOM_CHUNK_WORDS words of one branch: the scan carries the last
//                           start, the flank before it and the directions met since
// No block waits for another.  Integer adds commute and every edge record has one writer: the result depends on
// no launch shape.
#ifndef EPV_TRACTS_H
#define EPV_TRACTS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"
#include "epv_domains.h"
#include "epv_rows.h"
#include "epv_tract_rec.h"

// the classes a block can close: 3 directions x 2 left flanks x 2 right flanks (a flank "none" goes to a record)
#define EPV_TRACT_LOCAL 12u
#define EPV_TRACT_F_FLANK 3u   /* EpvTractCarry::f: bits 0-1 the flank before the start (2 = none) */
#define EPV_TRACT_F_GAIN 4u    /*                   bit 2 a gained site since the start */
#define EPV_TRACT_F_LOSS 8u    /*                   bit 3 a lost site since the start */

// what the scan carries: the last tract start so far as p + 1 (0 = none), and f
struct EpvTractCarry {
  uint32_t start, f;
};
// l lies before r
__device__ __forceinline__ EpvTractCarry epv_tract_join(EpvTractCarry l, EpvTractCarry r) {
  if (r.start) return r;
  l.f |= r.f & (EPV_TRACT_F_GAIN | EPV_TRACT_F_LOSS);
  return l;
}
// the flank of a start at bit sb of a word y whose first site is `base`; before = the word before it
__device__ __forceinline__ uint32_t epv_tract_flank(uint32_t sb, unsigned long long y, unsigned long long before,
                                                    uint32_t base) {
  if (base + sb == 0u) return EPV_TRACT_NONE;
  return (uint32_t)(sb ? y >> (sb - 1u) : before >> 63) & 1u;
}
// the carry of one word: c its changes, y its end states, st its starts
__device__ __forceinline__ EpvTractCarry epv_tract_word(unsigned long long c, unsigned long long y, unsigned long long st,
                                                        unsigned long long before, uint32_t base) {
  EpvTractCarry k = {0u, 0u};
  unsigned long long g = c & y, l = c & ~y;
  if (st) {
    const uint32_t sb = 63u - (uint32_t)__builtin_clzll(st);
    k.start = base + sb + 1u;
    k.f = epv_tract_flank(sb, y, before, base);
    g >>= sb;
    l >>= sb;
  }
  k.f |= (g ? EPV_TRACT_F_GAIN : 0u) | (l ? EPV_TRACT_F_LOSS : 0u);
  return k;
}
// the OR of v over the block's 256 threads, bits 2 and 3 alone (every thread gets it); red: 4 words of LDS
__device__ __forceinline__ uint32_t epv_tract_block_or(uint32_t v, uint32_t *red) {
  const uint32_t o = (__ballot(v & EPV_TRACT_F_GAIN) ? EPV_TRACT_F_GAIN : 0u) |
                     (__ballot(v & EPV_TRACT_F_LOSS) ? EPV_TRACT_F_LOSS : 0u);
  __syncthreads();   // (red may still be read from an earlier call)
  if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = o;
  __syncthreads();
  return red[0] | red[1] | red[2] | red[3];
}
// the global class of a local one (direction * 4 + left * 2 + right)
__device__ __forceinline__ uint32_t epv_tract_global_class(uint32_t local) {
  return epv_tract_class(local >> 2, (local >> 1) & 1u, local & 1u);
}

// grid (chunks, branches of this launch), 256 threads; branch = b0 + blockIdx.y, its rows 2 b and 2 b + 1 of bits.
// Positions are kept as p + 1 in 32 bits (0 = none): cnt < 2^32.  hist [B][27][128] and len_sum [B][27] take the
// tracts that start after the stretch's first site and end before its last; edge = this sample's records [B][2].
__global__ __launch_bounds__(256) void epv_tract_runs_kernel(const unsigned long long *bits, uint64_t words, uint64_t cnt,
                                                             uint32_t b0, unsigned long long *hist,
                                                             unsigned long long *len_sum, unsigned long long *edge) {
  __shared__ uint32_t table[EPV_TRACT_LOCAL * EPV_DOM_BINS];
  __shared__ unsigned long long sums[EPV_TRACT_LOCAL];
  __shared__ uint32_t red[4];
  __shared__ uint32_t wave_start[4], wave_f[4];
  const uint32_t t = threadIdx.x, b = b0 + blockIdx.y;
  const unsigned long long *rowa = bits + (uint64_t)(2u * b) * words, *rowy = rowa + words;
  const uint64_t c0 = (uint64_t)blockIdx.x * EPV_DOM_CHUNK_WORDS;   // the chunk's first word (< words)
#pragma unroll
  for (uint32_t h = 0; h < EPV_TRACT_LOCAL * EPV_DOM_BINS / 256u; ++h) table[t + 256u * h] = 0u;
  if (t < EPV_TRACT_LOCAL) sums[t] = 0ull;

  // this thread's words with the word before and the word after: changes cw, end states yw (index j + 1 = word
  // i0 + j; zero outside the row, and the pack kernel left zeros beyond cnt)
  const uint64_t i0 = c0 + (uint64_t)t * EPV_DOM_WPT;
  unsigned long long cw[EPV_DOM_WPT + 2u], yw[EPV_DOM_WPT + 2u];
#pragma unroll
  for (uint32_t j = 0; j < EPV_DOM_WPT + 2u; ++j) {
    const bool have = i0 + j >= 1u && i0 + j - 1u < words;
    const unsigned long long a = have ? rowa[i0 + j - 1u] : 0ull;
    yw[j] = have ? rowy[i0 + j - 1u] : 0ull;
    cw[j] = a ^ yw[j];
  }
  // starts, ends (below cnt - 1: the last site is an open end) and the carry of every word
  unsigned long long st[EPV_DOM_WPT], en[EPV_DOM_WPT];
  EpvTractCarry wc[EPV_DOM_WPT], own = {0u, 0u};
#pragma unroll
  for (uint32_t j = 0; j < EPV_DOM_WPT; ++j) {
    const unsigned long long c = cw[j + 1u];
    const uint64_t base = (i0 + j) * 64u;
    st[j] = c & ~((c << 1) | (cw[j] >> 63));
    unsigned long long e = c & ~((c >> 1) | (cw[j + 2u] << 63));
    if (base + 64u > cnt - 1u) e &= base >= cnt - 1u ? 0ull : (~0ull >> (64u - (uint32_t)(cnt - 1u - base)));
    en[j] = e;
    wc[j] = epv_tract_word(c, yw[j + 1u], st[j], yw[j], (uint32_t)base);
    own = epv_tract_join(own, wc[j]);
  }

  // carry-in, needed only when the site before the chunk changed: the start of its tract, looked for 256 words at a
  // time towards the row's start (site 0 is a start when it changed, so the search ends), and the directions of
  // the tract's sites up to the chunk
  EpvTractCarry carry = {0u, 0u};
  if (c0 > 0u && ((rowa[c0 - 1u] ^ rowy[c0 - 1u]) >> 63)) {   // (block-uniform)
    for (uint64_t hi = c0; hi > 0u && carry.start == 0u;) {   // (block-uniform: carry comes from block reductions)
      const uint64_t lo_w = hi > 256u ? hi - 256u : 0u, i = lo_w + t;
      uint32_t e = 0u, f = 0u;
      if (i < hi) {
        const unsigned long long y = rowy[i], c = rowa[i] ^ y;
        const unsigned long long cp = i ? rowa[i - 1u] ^ rowy[i - 1u] : 0ull;
        const EpvTractCarry k = epv_tract_word(c, y, c & ~((c << 1) | (cp >> 63)), 0ull, (uint32_t)(i * 64u));
        e = k.start;
        f = k.f;
      }
      const uint32_t m = epv_dom_block_max(e, red);
      // the words of the tract that starts at m: the word that holds it, and the words behind it (they hold no start)
      const bool counts = i < hi && (m == 0u || e == m || (e == 0u && i * 64u >= (uint64_t)m));
      carry.f |= epv_tract_block_or(counts ? f : 0u, red);
      carry.start = m;
      hi = lo_w;
    }
    carry.f &= EPV_TRACT_F_GAIN | EPV_TRACT_F_LOSS;
    const uint32_t q = carry.start - 2u;   // the site before the start (carry.start >= 1)
    carry.f |= carry.start <= 1u ? EPV_TRACT_NONE : (uint32_t)(rowy[q >> 6] >> (q & 63u)) & 1u;
  }

  // inclusive scan of the carries over the block: shuffles inside a wave, LDS across the four waves
  EpvTractCarry inc = own;
  const uint32_t lane = t & 63u, wave = t >> 6;
  for (int s = 1; s < 64; s <<= 1) {
    EpvTractCarry o;
    o.start = (uint32_t)__shfl_up((int)inc.start, (unsigned)s, 64);
    o.f = (uint32_t)__shfl_up((int)inc.f, (unsigned)s, 64);
    if (lane >= (uint32_t)s) inc = epv_tract_join(o, inc);
  }
  EpvTractCarry cur;   // exclusive, within the wave
  cur.start = (uint32_t)__shfl_up((int)inc.start, 1u, 64);
  cur.f = (uint32_t)__shfl_up((int)inc.f, 1u, 64);
  if (lane == 0u) cur.start = cur.f = 0u;
  if (lane == 63u) { wave_start[wave] = inc.start; wave_f[wave] = inc.f; }
  __syncthreads();   // (also: table and sums are zeroed)
  EpvTractCarry before = carry;
  for (uint32_t x = 0; x < wave; ++x) before = epv_tract_join(before, EpvTractCarry{wave_start[x], wave_f[x]});
  cur = epv_tract_join(before, cur);

  // walk the ends lowest first: the tract's start is the last start at or below the end, in this word or carried
  const unsigned long long y0 = rowy[0] & 1ull;
#pragma unroll
  for (uint32_t j = 0; j < EPV_DOM_WPT; ++j) {
    unsigned long long dd = en[j];
    const unsigned long long y = yw[j + 1u];
    const uint32_t base = (uint32_t)((i0 + j) * 64u);
    while (dd) {
      const uint32_t e = (uint32_t)__ffsll((long long)dd) - 1u;
      dd &= dd - 1ull;
      unsigned long long m = ~0ull >> (63u - e);   // the bits of this word that belong to the tract
      const unsigned long long sm = st[j] & m;
      uint32_t start = cur.start, f = cur.f;
      if (sm) {
        const uint32_t sb = 63u - (uint32_t)__builtin_clzll(sm);
        m &= ~0ull << sb;
        start = base + sb + 1u;
        f = epv_tract_flank(sb, y, yw[j], base);
      }
      const uint32_t gain = ((f & EPV_TRACT_F_GAIN) || (y & m)) ? 1u : 0u, loss = ((f & EPV_TRACT_F_LOSS) || (~y & m)) ? 1u : 0u;
      const uint32_t left = f & EPV_TRACT_F_FLANK, right = (uint32_t)(e < 63u ? y >> (e + 1u) : yw[j + 2u]) & 1u;
      const uint32_t len = base + e + 2u - start;
      if (left == EPV_TRACT_NONE) {   // the tract from the stretch's first site, which only a merge can close
        edge[(uint64_t)b * 2u] = EPV_TRACT_SET | (unsigned long long)len | (y0 << EPV_TRACT_Y_SHIFT) |
                                 ((unsigned long long)gain << EPV_TRACT_GAIN_SHIFT) |
                                 ((unsigned long long)loss << EPV_TRACT_LOSS_SHIFT) |
                                 ((unsigned long long)right << EPV_TRACT_FLANK_SHIFT);
      } else {
        const uint32_t cls = epv_tract_dir(gain, loss) * 4u + (left & 1u) * 2u + right;   // (< EPV_TRACT_LOCAL)
        atomicAdd(&table[cls * EPV_DOM_BINS + epv_domain_bin(len)], 1u);
        atomicAdd(&sums[cls], (unsigned long long)len);
      }
    }
    cur = epv_tract_join(cur, wc[j]);
  }

  // an unchanged first site: its record, from the row's first block
  if (blockIdx.x == 0u && t == 0u && !(cw[1] & 1ull)) edge[(uint64_t)b * 2u] = EPV_TRACT_SET | (y0 << EPV_TRACT_Y_SHIFT);
  // the row's last word is in this block: the record of the last site, or of the whole stretch
  if (c0 + EPV_DOM_CHUNK_WORDS >= words && t == 0u) {
    EpvTractCarry all = carry;
    for (uint32_t x = 0; x < 4u; ++x) all = epv_tract_join(all, EpvTractCarry{wave_start[x], wave_f[x]});
    const uint64_t q = cnt - 1u;
    const unsigned long long yl = (rowy[q >> 6] >> (q & 63u)) & 1ull, cl = ((rowa[q >> 6] >> (q & 63u)) & 1ull) ^ yl;
    const unsigned long long dirs = (unsigned long long)((all.f >> 2) & 3u) << EPV_TRACT_GAIN_SHIFT;
    if (!cl) {
      edge[(uint64_t)b * 2u + 1u] = EPV_TRACT_SET | (yl << EPV_TRACT_Y_SHIFT);
    } else if (all.start <= 1u) {
      edge[(uint64_t)b * 2u] = EPV_TRACT_SET | EPV_TRACT_WHOLE | cnt | dirs | (y0 << EPV_TRACT_Y_SHIFT);
      edge[(uint64_t)b * 2u + 1u] = EPV_TRACT_SET | EPV_TRACT_WHOLE | cnt | dirs | (yl << EPV_TRACT_Y_SHIFT);
    } else {
      edge[(uint64_t)b * 2u + 1u] = EPV_TRACT_SET | (cnt + 1u - all.start) | dirs | (yl << EPV_TRACT_Y_SHIFT) |
                                    ((unsigned long long)(all.f & 1u) << EPV_TRACT_FLANK_SHIFT);
    }
  }

  // flush: the nonzero cells and length sums
  __syncthreads();
#pragma unroll
  for (uint32_t h = 0; h < EPV_TRACT_LOCAL * EPV_DOM_BINS / 256u; ++h) {
    const uint32_t at = t + 256u * h, cell = table[at];
    if (cell)
      atomicAdd(hist + ((uint64_t)b * EPV_TRACT_CLASSES + epv_tract_global_class(at / EPV_DOM_BINS)) * EPV_DOM_BINS +
                    (at & (EPV_DOM_BINS - 1u)), (unsigned long long)cell);
  }
  if (t < EPV_TRACT_LOCAL && sums[t]) atomicAdd(len_sum + (uint64_t)b * EPV_TRACT_CLASSES + epv_tract_global_class(t), sums[t]);
}

#endif
