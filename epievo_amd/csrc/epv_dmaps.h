// epv_dmaps.h -- domain maps: per node, size and site, the number of sampled histories in which the site lies in a
// run of state s of at least L_k sites (K <= 4 sizes, L_1 < .. < L_K <= 1024).  The located counterpart of the
// domain size spectra (epv_domains.h), joint along the genome like them: a run can cross any chunk, context or GPU
// boundary, so a context counts a PART (include/epievo_mi355x.h, epv_set_domain_maps): counts [N][K][cnt] with the
// runs clipped to its stretch, and per sample and node the first and the last E = 2 (L_K - 1) bits of the node's
// row as edge records.  Parts are merged on the host (host/epv_dmaps.cpp); there is no close step.
//
// A row is the indicator of "x_v = s" (x_v as the domain size spectra define it, from the 16-bit meta word alone).
// Membership is a morphological opening of the row: erode by L (a bit stays where a run of L ones starts), then
// dilate by L (every site of such a run).
//
// Two launches per sample:
//   epv_rows_pack_kernel      the node rows of the state to indicate (epv_rows.h) -> bits[v][tile]
//   epv_dmaps_member_kernel   one block per chunk of EPV_DMAPS_CHUNK_WORDS words of one node's row: the chunk and a
//                             halo on either side are held a word (or two) per thread and exchanged through LDS for
//                             every shifted AND / OR; spans double, and the erosion of a size continues that of the
//                             size before.  Then a lane per site adds 1 where its bit is set.  The first and the
//                             last chunk's block write the row's edge records
// The exchange buffer is double: a step writes one half, waits once, reads it; the next step takes the other half,
// so no thread overwrites what a slower one still reads.  Consecutive threads hold consecutive 8-byte words: the
// shifted reads (w[i + q], w[i + q + 1]) are consecutive too, without bank conflicts.
// No block waits for another; every counter and every record word has one writer; there are no atomics.
#ifndef EPV_DMAPS_H
#define EPV_DMAPS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"
#include "epv_domains.h"
#include "epv_rows.h"

#define EPV_DMAPS_MAX_SIZE 1024u
#define EPV_DMAPS_MAX_SIZES 4u
#define EPV_DMAPS_MAX_SAMPLES (1ull << 21)
/* words of a row per block of the membership kernel: 16 384 sites (measured once, not tuned).  A row of 10^6 sites
 * is 15 625 words: 62 blocks per row, 1922 over the 31 rows of the 16-leaf tree */
#define EPV_DMAPS_CHUNK_WORDS 256u
#define EPV_DMAPS_MAX_HALO ((EPV_DMAPS_MAX_SIZE - 1u + 63u) / 64u + 1u)
#define EPV_DMAPS_STAGE_WORDS (EPV_DMAPS_CHUNK_WORDS + 2u * EPV_DMAPS_MAX_HALO)   /* <= 2 x 256: two words a thread */
#define EPV_DMAPS_MAX_EDGE_WORDS ((2u * (EPV_DMAPS_MAX_SIZE - 1u) + 63u) / 64u)

struct EpvDmapSizes {
  uint32_t K;                          // 1 .. EPV_DMAPS_MAX_SIZES
  uint32_t L[EPV_DMAPS_MAX_SIZES];     // strictly increasing, 1 .. EPV_DMAPS_MAX_SIZE
};

// word i of the staged string, zero outside it
__device__ __forceinline__ unsigned long long epv_dmaps_at(const unsigned long long *w, uint32_t total, int32_t i) {
  return i >= 0 && (uint32_t)i < total ? w[i] : 0ull;
}
// word i of the string shifted down by step bits (bit p of the result = bit p + step), 1 <= step
__device__ __forceinline__ unsigned long long epv_dmaps_down(const unsigned long long *w, uint32_t total, uint32_t i,
                                                             uint32_t step) {
  const int32_t j = (int32_t)(i + (step >> 6));
  const uint32_t s = step & 63u;   // (no shift by 64 is formed)
  return (epv_dmaps_at(w, total, j) >> s) | ((epv_dmaps_at(w, total, j + 1) << 1) << (63u - s));
}
// word i of the string shifted up by step bits (bit p of the result = bit p - step), 1 <= step
__device__ __forceinline__ unsigned long long epv_dmaps_up(const unsigned long long *w, uint32_t total, uint32_t i,
                                                           uint32_t step) {
  const int32_t j = (int32_t)i - (int32_t)(step >> 6);
  const uint32_t s = step & 63u;
  return (epv_dmaps_at(w, total, j) << s) | ((epv_dmaps_at(w, total, j - 1) >> 1) >> (63u - s));
}

// grid (chunks, nodes of this launch), 256 threads; row = v0 + blockIdx.y.  counts [N][K][cnt] (uint32); edge = this
// sample's records [N][2][EW], EW = ceil(E / 64), E = 2 (L_K - 1) <= cnt: the head is written by the block of the
// first chunk, the tail (the E bits that end at cnt) by the block of the last.  Bits beyond cnt are zero in `bits`,
// and an opening sets no bit that was not set: no site beyond cnt is counted.
__global__ __launch_bounds__(256) void epv_dmaps_member_kernel(const unsigned long long *bits, uint64_t words, uint64_t cnt,
                                                               uint32_t v0, EpvDmapSizes Z, uint32_t *counts,
                                                               unsigned long long *edge) {
  __shared__ unsigned long long buf[2][EPV_DMAPS_STAGE_WORDS];
  const uint32_t t = threadIdx.x, v = v0 + blockIdx.y;
  const unsigned long long *row = bits + (uint64_t)v * words;
  const uint64_t c0 = (uint64_t)blockIdx.x * EPV_DMAPS_CHUNK_WORDS;   // the chunk's first word (< words)
  const uint32_t K = Z.K, LK = Z.L[K - 1u];
  const uint32_t H = (LK - 1u + 63u) / 64u + 1u;   // halo words on either side (<= EPV_DMAPS_MAX_HALO)
  const uint32_t nw = (uint32_t)(words - c0 < EPV_DMAPS_CHUNK_WORDS ? words - c0 : EPV_DMAPS_CHUNK_WORDS);
  const uint32_t total = nw + 2u * H;              // (<= EPV_DMAPS_STAGE_WORDS); slot i = word c0 - H + i of the row
  const uint32_t own[2] = {t, t + 256u};

  // the erosion so far (span a), a word or two per thread; words beyond the stretch are zero
  unsigned long long e[2];
#pragma unroll
  for (uint32_t j = 0; j < 2u; ++j) {
    const uint64_t g = c0 + own[j];   // (word g - H of the row)
    e[j] = own[j] < total && g >= H && g - H < words ? row[g - H] : 0ull;
  }
  uint32_t pp = 0u, a = 1u;
  for (uint32_t k = 0; k < K; ++k) {   // (every loop bound below is the same for the whole block)
    const uint32_t L = Z.L[k];
    while (a < L) {
      const uint32_t step = a < L - a ? a : L - a;
      unsigned long long *w = buf[pp];
      pp ^= 1u;
#pragma unroll
      for (uint32_t j = 0; j < 2u; ++j) if (own[j] < total) w[own[j]] = e[j];
      __syncthreads();
#pragma unroll
      for (uint32_t j = 0; j < 2u; ++j) if (own[j] < total) e[j] &= epv_dmaps_down(w, total, own[j], step);
      a += step;
    }
    unsigned long long d[2] = {e[0], e[1]};
    for (uint32_t b = 1u; b < L;) {
      const uint32_t step = b < L - b ? b : L - b;
      unsigned long long *w = buf[pp];
      pp ^= 1u;
#pragma unroll
      for (uint32_t j = 0; j < 2u; ++j) if (own[j] < total) w[own[j]] = d[j];
      __syncthreads();
#pragma unroll
      for (uint32_t j = 0; j < 2u; ++j) if (own[j] < total) d[j] |= epv_dmaps_up(w, total, own[j], step);
      b += step;
    }
    // the chunk's membership words to LDS; a wave takes every fourth word, a lane a site
    unsigned long long *w = buf[pp];
    pp ^= 1u;
#pragma unroll
    for (uint32_t j = 0; j < 2u; ++j) if (own[j] < total) w[own[j]] = d[j];
    __syncthreads();
    uint32_t *out = counts + ((uint64_t)v * K + k) * cnt;
    const uint32_t lane = t & 63u;
    for (uint32_t i = t >> 6; i < nw; i += 4u) {
      const unsigned long long m = w[H + i];   // (one address per wave: a broadcast)
      const uint64_t site = (c0 + i) * 64u + lane;
      if (((m >> lane) & 1ull) && site < cnt) out[site] += 1u;
    }
  }

  // edge records: word j of the head = bits 64 j .. of the row, of the tail = bits cnt - E + 64 j ..; the spare bits
  // of the last word are zero
  const uint32_t E = 2u * (LK - 1u), EW = (E + 63u) >> 6;
  if (!EW) return;
  const unsigned long long last_mask = (E & 63u) ? ~0ull >> (64u - (E & 63u)) : ~0ull;
  unsigned long long *rec = edge + (uint64_t)v * 2u * EW;
  if (blockIdx.x == 0u && t < EW) {
    const unsigned long long x = t < words ? row[t] : 0ull;
    rec[t] = t + 1u == EW ? x & last_mask : x;
  }
  if (c0 + EPV_DMAPS_CHUNK_WORDS >= words && t < EW) {
    const uint64_t st = cnt - E, i = (st >> 6) + t;
    const uint32_t s = (uint32_t)(st & 63u);
    const unsigned long long lo = i < words ? row[i] : 0ull, hi = i + 1u < words ? row[i + 1u] : 0ull;
    const unsigned long long x = (lo >> s) | ((hi << 1) << (63u - s));
    rec[EW + t] = t + 1u == EW ? x & last_mask : x;
  }
}

#endif
