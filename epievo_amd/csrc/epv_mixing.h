// epv_mixing.h -- chain mixing diagnostics: does a site's history move from one sample to the next, and how
// long does its jump count remember itself.  Per site s of the sites a context counts, over the samples:
//   h_t  the whole history on the tree: for every branch the meta word (init state, number of jumps) and the
//        bit pattern of every jump time, read from the buffer sel[s] points to
//   x_t  the jumps of the site over all branches (its share of J)
//   moved  linked sample pairs (t - 1, t) with h_t != h_{t-1}
//   S1 = sum x_t, S2 = sum x_t^2, C_k = sum x_t x_{t-k} over linked pairs at lag k = 1 .. K
// h_t is compared through a 64-bit fingerprint kept per site: the sum over the branches b and the jumps j of
// mix(word ^ key(b, j)), so the same times on another branch or in another order give another sum.  Two
// different histories collide with probability 2^-64; a collision undercounts one move.
// Buffers, SoA over the counted sites (sites fastest): fp u64 [cnt], moved u32 [cnt], sums u64 [2 + K][cnt]
// (S1, S2, C_1 .. C_K), ring u32 [K][cnt] (the site's last K values of x).  x <= B C < 2^23, and the host caps
// the samples so that no sum wraps.  Every site has one owner thread: plain loads and stores, no atomics.
#ifndef EPV_MIXING_H
#define EPV_MIXING_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"

#define EPV_MIX_MAX_LAG 16u
#define EPV_MIX_MAX_SAMPLES (1ull << 21)
#define EPV_MIX_BCH 8u   /* branches whose meta loads are in flight together */

// what a sample is to the run it belongs to (the host keeps the run: DESIGN.md section 7.19)
#define EPV_MIX_OPEN 0u     /* the opening state of a run: its fingerprint is stored, nothing is counted */
#define EPV_MIX_FIRST 1u    /* a sample that opens a run itself: counted, linked to nothing */
#define EPV_MIX_LINKED 2u   /* a sample linked to its predecessor */

// the finalizer of splitmix64: a bijection of 64-bit words
__device__ __forceinline__ uint64_t epv_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// one thread per site of lo .. lo + cnt - 1: sel once, the current buffer's meta words of all branches,
// EPV_MIX_BCH loads at a time, then the jump times of the branches that have any (lanes = sites: a wave's
// loads of one (branch, jump) are contiguous).  slot < K is where x goes in the ring, lags <= K how many
// earlier samples of the run the ring holds: sample t - k sits at slot - k (mod K)
__global__ __launch_bounds__(256) void epv_mixing_accum_kernel(EpvDev S, uint64_t lo, uint64_t cnt, uint32_t K,
                                                               uint32_t mode, uint32_t slot, uint32_t lags,
                                                               unsigned long long *fp, uint32_t *moved,
                                                               unsigned long long *sums, uint32_t *ring) {
  const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (s >= cnt) return;
  const uint64_t site = lo + s, n = S.n;
  const uint32_t B = S.B, C = S.C;
  const uint32_t buf = S.sel[site];
  const epv_meta_t *m = S.meta + (buf ? (uint64_t)B * n : 0ull) + site;
  const double *jbase = S.jumps + (buf ? (uint64_t)B * C * n : 0ull) + site;
  uint64_t h = 0;
  uint32_t x = 0;
  for (uint32_t b0 = 0; b0 < B; b0 += EPV_MIX_BCH) {
    uint32_t w[EPV_MIX_BCH];
#pragma unroll
    for (uint32_t i = 0; i < EPV_MIX_BCH; ++i) w[i] = b0 + i < B ? (uint32_t)m[(uint64_t)(b0 + i) * n] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < EPV_MIX_BCH; ++i) {
      if (b0 + i >= B) break;
      const uint64_t key = epv_mix64((uint64_t)(b0 + i) + 1u);   // (of the branch; jump j takes key + (j + 1) odd)
      h += epv_mix64((uint64_t)w[i] ^ key);
      const uint32_t nj = w[i] & EPV_NJ_MASK;
      if (!nj) continue;
      x += nj;
      const double *j = jbase + (uint64_t)(b0 + i) * C * n;
      for (uint32_t k = 0; k < nj; ++k)
        h += epv_mix64((uint64_t)__double_as_longlong(j[(uint64_t)k * n]) ^ (key + (uint64_t)(k + 1u) * 0x9e3779b97f4a7c15ull));
    }
  }
  const uint64_t before = fp[s];
  fp[s] = h;
  if (mode == EPV_MIX_OPEN) return;
  if (mode == EPV_MIX_LINKED && before != h) moved[s] += 1u;
  if (x) {
    sums[s] += x;
    sums[cnt + s] += (uint64_t)x * x;
    for (uint32_t k = 1; k <= lags; ++k) {
      const uint32_t at = slot >= k ? slot - k : slot + K - k;
      const uint32_t y = ring[(uint64_t)at * cnt + s];
      if (y) sums[(uint64_t)(1u + k) * cnt + s] += (uint64_t)x * y;
    }
  }
  ring[(uint64_t)slot * cnt + s] = x;
}

#endif
