// epv_wstat.h -- regional sufficient statistics: the exact integers of epv_suffstat_wave_kernel (J as
// counts, every dwell time as rint(dt * 2^k_b)), split by genomic window.  Window w = global sites
// [w W, (w + 1) W); a triple belongs to the window of its centre site.  A sample adds to
// acc[local window][b][16] (uint64: J[8], D[8]), local window 0 = the window of the first owned site.
// Integer sums commute: the result depends on no launch shape, on no order in which additions land,
// and not on how W relates to the 64-site tile.  Every device addition is a 64-bit vector atomic.
//
// One wave per block, 64 consecutive sites from the first owned site, up to EPV_WSTAT_BCH branches: the
// shape of epv_suffstat_wave_kernel, whose stages it keeps -- the neighbours' meta words through LDS,
// the no-jump triples as a ballot/popcount histogram, the others queued in an LDS ring and merged
// with dense lanes by merge3.  What differs is where an event lands:
//   WIDE (W >= 64): a tile meets at most two windows, the lanes below `nlow` and the others.  Two LDS
//     accumulator sets; the histogram masks its ballot with either half; a merged pair adds into the
//     set of its centre lane.  Nonzero words are flushed once, at the end.
//   SMALL (W < 64): up to 64 windows per tile.  A merged pair adds straight into its window's global
//     row (those are the rare pairs).  The no-jump triples are counted per (window of the tile,
//     context) in a 2 KB LDS table, one branch at a time, and each nonzero cell leaves as ONE global
//     add of count * fix(T_b): W-fold fewer global atomics than an add per lane, and no pass per
//     window (64 ballot passes per branch at W = 1).  Only the cells of the windows the tile meets
//     are scanned (8 per window: 512 at W = 1, 24 at W = 32).
// LDS of a block: 4.0 KB (WIDE), 3.5 KB (SMALL) -- a third of the ~11 KB the colour phases leave free.
#ifndef EPV_WSTAT_H
#define EPV_WSTAT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"
#include "epv_kernels.h"

#define EPV_WSTAT_BCH 8u

// merge3's accumulator: the 16 words (LDS or global) of the window that holds the triple's centre site
struct AccWin {
  unsigned long long *acc;
  double scale;              // 2^k_b
};
__device__ __forceinline__ void acc_add(AccWin &A, int ctx, double dt, bool mid) {
  atomicAdd(&A.acc[8 + ctx], epv_stat_fix(dt, A.scale));
  if (mid) atomicAdd(&A.acc[ctx], 1ull);
}

// first .. last: the owned local sites (tiles start at `first`); w_first: the global window of site
// `first`; n_lw: local windows in acc
template <bool SMALL>
__global__ __launch_bounds__(64) void epv_wstat_accum_kernel(EpvDev S, uint64_t first, uint64_t last,
                                                             const double *statscale, uint64_t W, uint64_t w_first,
                                                             uint64_t n_lw, unsigned long long *acc) {
  __shared__ unsigned long long s_acc[SMALL ? 1u : 2u * EPV_WSTAT_BCH * 16u];
  __shared__ uint32_t s_cnt[SMALL ? 512u : 2u * EPV_WSTAT_BCH * 8u];   // SMALL: [window of the tile][context]
  __shared__ epv_meta_t s_meta[66];
  __shared__ uint8_t s_sel[66];
  __shared__ uint8_t s_lw[64];          // SMALL: a lane's window, relative to the tile's first
  __shared__ uint32_t s_ring[128], s_ring_lm[128];
  __shared__ epv_meta_t s_ring_r[128];
  const uint32_t t = threadIdx.x;
  const int lane = (int)t;
  const uint32_t B = S.B;
  const uint32_t b_lo = blockIdx.y * EPV_WSTAT_BCH, b_hi = (b_lo + EPV_WSTAT_BCH < B) ? b_lo + EPV_WSTAT_BCH : B;
  const uint64_t n = S.n, Bn = (uint64_t)B * n, Cn = (uint64_t)S.C * n;
  const uint64_t site0 = first + (uint64_t)blockIdx.x * 64u, site = site0 + t;
  const bool on = site <= last && site >= 1 && site + 1 < n;
  // the tile's first window and how many of its sites lie in it (wave-uniform: one 64-bit division)
  const uint64_t gw0 = (S.g0 + site0) / W, lw0 = gw0 - w_first;
  const uint64_t in0 = (gw0 + 1u) * W - (S.g0 + site0);             // >= 1
  const uint32_t nlow = in0 < 64u ? (uint32_t)in0 : 64u;
  const unsigned long long lowmask = nlow >= 64u ? ~0ull : ((1ull << nlow) - 1ull);
  const uint32_t my_lw = SMALL ? (t < nlow ? 0u : 1u + (t - nlow) / (uint32_t)W) : (t < nlow ? 0u : 1u);
  // SMALL: the table cells of the windows this tile meets (wave-uniform, <= 512: 24 at W = 32, all at W = 1)
  const uint32_t ncell = SMALL ? 8u * (1u + (64u - nlow + (uint32_t)W - 1u) / (uint32_t)W) : 0u;
  const uint32_t my_sel = site < n ? S.sel[site] : 0u;
  const bool edge = (t == 0 && site0 >= 1) || (t == 1 && site0 + 64u < n);
  const uint64_t esite = t == 0 ? site0 - 1 : site0 + 64u;
  const uint32_t e_sel = edge ? S.sel[esite] : 0u;
  if constexpr (SMALL) {
    for (uint32_t i = t; i < 512u; i += 64u) s_cnt[i] = 0u;
    s_lw[t] = (uint8_t)my_lw;
  } else {
    for (uint32_t i = t; i < 2u * EPV_WSTAT_BCH * 16u; i += 64u) s_acc[i] = 0ull;
    s_cnt[t] = 0u;
    s_cnt[t + 64u] = 0u;
  }
  s_sel[t + 1u] = (uint8_t)my_sel;
  if (t < 2u) s_sel[t == 0 ? 0 : 65] = (uint8_t)e_sel;
  const uint64_t mbase = (my_sel ? Bn : 0ull) + site;
  const uint64_t ebase = (e_sel ? Bn : 0ull) + esite;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();

  auto merge_item = [&](uint32_t slot) __attribute__((always_inline)) {
    const uint32_t item = s_ring[slot], lm = s_ring_lm[slot], mr = s_ring_r[slot];
    const uint32_t ti = item & 63u, bl = item >> 8, b = b_lo + bl;
    const uint64_t si = site0 + ti;
    const uint32_t ml = lm & 0xffffu, mm = lm >> 16;
    PathRef L, M, R;
    L.j = S.jumps + (s_sel[ti] ? Bn * S.C : 0ull) + (uint64_t)b * Cn + (si - 1); L.nj = ml & EPV_NJ_MASK; L.init = ml >> EPV_INIT_SHIFT;
    M.j = S.jumps + (s_sel[ti + 1u] ? Bn * S.C : 0ull) + (uint64_t)b * Cn + si; M.nj = mm & EPV_NJ_MASK; M.init = mm >> EPV_INIT_SHIFT;
    R.j = S.jumps + (s_sel[ti + 2u] ? Bn * S.C : 0ull) + (uint64_t)b * Cn + (si + 1); R.nj = mr & EPV_NJ_MASK; R.init = mr >> EPV_INIT_SHIFT;
    AccWin A;
    if constexpr (SMALL) {
      const uint64_t lw = lw0 + s_lw[ti];
      if (lw >= n_lw) return;          // (an owned site's window is a local one: never taken)
      A.acc = acc + (lw * B + b) * 16u;
    } else {
      A.acc = s_acc + ((ti < nlow ? 0u : 1u) * EPV_WSTAT_BCH + bl) * 16u;
    }
    A.scale = statscale[b + 1u];
    merge3(L, M, R, n, S.blen[b + 1u], A);
  };

  uint32_t head = 0u, tail = 0u;     // wave-uniform
  constexpr uint32_t GB = 4u;
  for (uint32_t b0 = b_lo; b0 < b_hi; b0 += GB) {
    epv_meta_t mq[GB], eq[GB];
#pragma unroll
    for (uint32_t q = 0; q < GB; ++q) {
      const bool have = b0 + q < b_hi;
      mq[q] = (have && site < n) ? S.meta[mbase + (uint64_t)(b0 + q) * n] : (epv_meta_t)0;
      eq[q] = (have && edge) ? S.meta[ebase + (uint64_t)(b0 + q) * n] : (epv_meta_t)0;
    }
#pragma unroll
    for (uint32_t q = 0; q < GB; ++q) {
      const uint32_t b = b0 + q;
      if (b >= b_hi) break;
      const uint32_t m = mq[q];
      s_meta[t + 1u] = (epv_meta_t)m;
      if (t < 2u) s_meta[t == 0 ? 0 : 65] = eq[q];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint32_t ml = s_meta[t], mr = s_meta[t + 2u];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();     // everybody has read: the next branch may overwrite
      const uint32_t or3 = (ml | m | mr) & EPV_NJ_MASK;
      const bool fast = on && or3 == 0u, slow = on && or3 != 0u;
      if constexpr (SMALL) {
        const uint32_t ctx = 4u * (ml >> EPV_INIT_SHIFT) + 2u * (m >> EPV_INIT_SHIFT) + (mr >> EPV_INIT_SHIFT);
        if (fast) atomicAdd(&s_cnt[my_lw * 8u + ctx], 1u);
      } else {
        const unsigned long long mf = __ballot(fast), m2 = __ballot((ml >> EPV_INIT_SHIFT) != 0u),
                                 m1 = __ballot((m >> EPV_INIT_SHIFT) != 0u), m0 = __ballot((mr >> EPV_INIT_SHIFT) != 0u);
        if (lane < 8) {
          const unsigned long long x = mf & ((lane & 4) ? m2 : ~m2) & ((lane & 2) ? m1 : ~m1) & ((lane & 1) ? m0 : ~m0);
          s_cnt[(b - b_lo) * 8u + (uint32_t)lane] += (uint32_t)__popcll(x & lowmask);     // this lane's own counters
          s_cnt[(EPV_WSTAT_BCH + b - b_lo) * 8u + (uint32_t)lane] += (uint32_t)__popcll(x & ~lowmask);
        }
      }
      const unsigned long long ms = __ballot(slow);
      if (slow) {
        const uint32_t slot = (tail + (uint32_t)__popcll(ms & ((1ull << lane) - 1ull))) & 127u;
        s_ring[slot] = t | ((b - b_lo) << 8);
        s_ring_lm[slot] = ml | (m << 16);
        s_ring_r[slot] = (epv_meta_t)mr;
      }
      tail += (uint32_t)__popcll(ms);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if constexpr (SMALL) {
        // this branch's table: a nonzero cell is one global add, and is zero again for the next branch
        const unsigned long long fixT = epv_stat_fix(S.blen[b + 1u] - 0.0, statscale[b + 1u]);
        for (uint32_t i = t; i < ncell; i += 64u) {
          const uint32_t v = s_cnt[i];
          if (!v) continue;
          s_cnt[i] = 0u;
          const uint64_t lw = lw0 + (i >> 3);
          if (lw < n_lw) atomicAdd(&acc[(lw * B + b) * 16u + 8u + (i & 7u)], (unsigned long long)v * fixT);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
      if (tail - head >= 64u) {
        merge_item((head + t) & 127u);
        head += 64u;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
      }
    }
  }
  if (t < tail - head) merge_item((head + t) & 127u);
  if constexpr (!SMALL) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = t; i < 2u * EPV_WSTAT_BCH * 16u; i += 64u) {
      const uint32_t half = i >> 7, bl = (i >> 4) & 7u, c = i & 15u, b = b_lo + bl;
      if (b >= b_hi) continue;
      unsigned long long v = s_acc[i];
      if (c >= 8u)
        v += (unsigned long long)s_cnt[(half * EPV_WSTAT_BCH + bl) * 8u + (c - 8u)] *
             epv_stat_fix(S.blen[b + 1u] - 0.0, statscale[b + 1u]);
      const uint64_t lw = lw0 + half;
      if (v && lw < n_lw) atomicAdd(&acc[(lw * B + b) * 16u + c], v);
    }
  }
}

#endif
