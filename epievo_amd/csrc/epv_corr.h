// epv_corr.h -- spatial correlations: for every node's state row and every branch's net-change row, the number of
// site pairs (p, p + d) that are both 1, for every lag d = 0 .. L (L = max_lag <= EPV_CORR_MAX_LAG), counted over the
// sampled histories.  Joint along the genome like the domain layers (epv_domains.h, epv_turnover.h): a pair can
// cross any chunk, context or GPU boundary, so a context counts a PART (include/epievo_mi355x.h,
// epv_set_spatial_correlation): the pairs inside its stretch in n11, and per sample and row the first and the last
// L bits of the stretch as edge records.  Parts are merged and closed on the host (host/epv_corr.cpp).
//
// Rows of one sample, from the 16-bit meta word alone (no jump time is read): R = N + B.  Row v < N is the state of
// node v as the domain size spectra define it (x_0 = the init state of the branch of the root's lowest-numbered
// child, x_v = a XOR (k & 1)); row N + b is the net change of branch b, k & 1.
//
// Two launches per sample:
//   epv_rows_pack_kernel    the node rows of state 1, then the change rows (epv_rows.h) -> bits[r][tile]
//   epv_corr_count_kernel   one block per chunk of EPV_CORR_CHUNK_WORDS words of one row: the chunk and the words
//                           a pair that starts in it can reach are staged in LDS; a thread owns lags and walks the
//                           chunk's words with a shifted AND and a popcount.  The first and the last chunk's block
//                           write the row's edge records
// A thread's lags are consecutive across a wave, so the LDS words it reads are the same for all lanes (w[i]) or one
// of two neighbours (w[i + q], q = d / 64): broadcasts, no bank conflicts.
// No block waits for another.  Integer adds commute and every edge word has one writer: the result depends on no
// launch shape.
#ifndef EPV_CORR_H
#define EPV_CORR_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"
#include "epv_domains.h"
#include "epv_rows.h"

#define EPV_CORR_MAX_LAG 1024u
#define EPV_CORR_MAX_LW (EPV_CORR_MAX_LAG / 64u)
#define EPV_CORR_MAX_SAMPLES (1ull << 21)
/* words of a row per block of the count kernel: 16 384 sites.  A row of 10^6 sites is 15 625 words: 62 blocks per
 * row, 558 over the 9 rows of a 5-node tree, for 256 CUs (1024 words would leave 16 per row) */
#define EPV_CORR_CHUNK_WORDS 256u
#define EPV_CORR_STAGE_WORDS (EPV_CORR_CHUNK_WORDS + EPV_CORR_MAX_LW + 1u)

// bits s .. s + 63 of the 128-bit string (a low, b high), 0 <= s < 64; no shift by 64 is formed
__device__ __forceinline__ unsigned long long epv_corr_window(unsigned long long a, unsigned long long b, uint32_t s) {
  return (a >> s) | ((b << 1) << (63u - s));
}

// grid (chunks, rows of this launch), up to 256 threads; row = r0 + blockIdx.y.  n11 [R][L + 1] takes the pairs whose
// left site lies in the chunk; bits beyond cnt are zero, so a pair that would leave the stretch counts nothing.
// edge = this sample's records [R][2][LW], LW = ceil(L / 64): the head is written by the block of the first chunk,
// the tail (the L bits that end at cnt, cnt >= L) by the block of the last.
__global__ __launch_bounds__(256) void epv_corr_count_kernel(const unsigned long long *bits, uint64_t words, uint64_t cnt,
                                                             uint32_t r0, uint32_t L, unsigned long long *n11,
                                                             unsigned long long *edge) {
  __shared__ unsigned long long w[EPV_CORR_STAGE_WORDS];
  const uint32_t t = threadIdx.x, r = r0 + blockIdx.y;
  const unsigned long long *row = bits + (uint64_t)r * words;
  const uint64_t c0 = (uint64_t)blockIdx.x * EPV_CORR_CHUNK_WORDS;   // the chunk's first word (< words)
  const uint32_t LW = (L + 63u) >> 6;
  const uint32_t nw = (uint32_t)(words - c0 < EPV_CORR_CHUNK_WORDS ? words - c0 : EPV_CORR_CHUNK_WORDS);
  const uint32_t stage = nw + LW + 1u;   // (<= EPV_CORR_STAGE_WORDS)
  for (uint32_t i = t; i < stage; i += blockDim.x) w[i] = c0 + i < words ? row[c0 + i] : 0ull;
  __syncthreads();

  for (uint32_t d = t; d <= L; d += blockDim.x) {
    const uint32_t q = d >> 6, s = d & 63u;   // (q <= LW: i + q + 1 < stage)
    uint32_t count = 0u;
    unsigned long long a = w[q];
    for (uint32_t i = 0; i < nw; ++i) {
      const unsigned long long b = w[i + q + 1u];
      count += (uint32_t)__popcll(w[i] & epv_corr_window(a, b, s));
      a = b;
    }
    if (count) atomicAdd(n11 + (uint64_t)r * (L + 1u) + d, (unsigned long long)count);
  }

  // edge records: word j of the head = bits 64 j .. of the row, of the tail = bits cnt - L + 64 j ..; the spare bits
  // of the last word are zero
  const unsigned long long last_mask = (L & 63u) ? ~0ull >> (64u - (L & 63u)) : ~0ull;
  unsigned long long *rec = edge + (uint64_t)r * 2u * LW;
  if (blockIdx.x == 0u && t < LW) {
    const unsigned long long x = t < words ? row[t] : 0ull;
    rec[t] = t + 1u == LW ? x & last_mask : x;
  }
  if (c0 + EPV_CORR_CHUNK_WORDS >= words && t < LW) {
    const uint64_t st = cnt - L, i = (st >> 6) + t;
    const unsigned long long a = i < words ? row[i] : 0ull, b = i + 1u < words ? row[i + 1u] : 0ull;
    const unsigned long long x = epv_corr_window(a, b, (uint32_t)(st & 63u));
    rec[LW + t] = t + 1u == LW ? x & last_mask : x;
  }
}

#endif
