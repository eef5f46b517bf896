// epv_epochs.h -- epoch statistics: the exact integers of the whole-genome statistics (J as counts, every
// dwell time as F = epv_stat_fix(dt, 2^k_b)), split by WHEN inside the branch they happened.  Everything
// lives on the triple's own fixed-point clock c (the running sum of its F), so the result is integers:
//   fixT = epv_stat_fix(T_b, 2^k_b);  edges E_p = floor(p fixT / P), p = 0 .. P-1, E_P = +inf;
//   bin(c) = the largest p <= P-1 with E_p <= c.
// An interval [c0, c1) of context ctx adds its overlap with [E_p, E_p+1) to D[p][ctx]; a jump of the
// centre site at its end adds 1 to J[bin(c1)][ctx].  An interval that spans the bins p0 < p1 costs four
// additions, not p1 - p0, in a difference form that is linear (so it adds over blocks, contexts and GPUs
// as integers) and is closed once on the host (host/epv_epochs.cpp):
//   part[p][ctx]: the pieces of the two end bins, E_{p0+1} - c0 and c1 - E_{p1} (F when p0 == p1);
//   cov[p][ctx]:  +1 at p0 + 1 and -1 at p1, so the prefix sum over p counts the intervals that cover
//                 bin p wholly;  D[p] = part[p] + (E_{p+1} - E_p) prefix(cov)[p].
// Global accumulator acc[b][p][32] (uint64): J[8], lo[8], hi[8], cov[8] (cov two's complement).  A block's
// 64-bit part sum v leaves as v & 0xffffffff into lo and v >> 32 into hi: every global word receives at
// most one addend below 2^32 per block and sample, which is what the host's cap counts.
//
// One block = one branch (blockIdx.y) over `tiles` tiles of 256 consecutive sites from the first owned
// site, so one branch's table is live in LDS at a time: part 64 P, J 32 P, cov 32 P bytes and the edge
// row 8 P (dynamic shared memory, 136 P bytes: 34 KB at P = EPV_EPOCH_MAX_P).  The stages are those of
// epv_suffstat_kernel: a lane loads its site's meta word, the neighbours' come through LDS; triples
// without a jump are a ballot/popcount histogram of the context, expanded as count x [0, fixT) at the
// flush; the others are queued in an LDS ring and walked with dense lanes, 256 at a time.  bin(c) is one
// fp64 estimate c P / fixT corrected against the edge row in either direction (the estimate decides
// nothing: the edges do).  Only nonzero cells flush, as 64-bit vector atomics.
#ifndef EPV_EPOCHS_H
#define EPV_EPOCHS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"
#include "epv_kernels.h"

#ifndef EPV_EPOCH_MAX_P
#define EPV_EPOCH_MAX_P 256u            // (include/epievo_mi355x.h)
#endif
#define EPV_EPOCH_MAX_TILES 32u     // 8192 sites x (fixT + 3072) < 2^64: a block's part sums cannot wrap
#define EPV_EPOCH_RING 512u        // at most 255 waiting + 256 new items

// one branch's table in LDS
struct EpochTab {
  unsigned long long *part;        // [P][8]
  uint32_t *J;                     // [P][8]
  int *cov;                        // [P][8]
  const unsigned long long *E;     // [P]
  uint32_t P;
  double inv_w;                    // P / fixT (0 when fixT == 0)
};

// bin(c) for c >= E[from]: the estimate, then the edges
__device__ __forceinline__ uint32_t epoch_bin(const EpochTab &T, unsigned long long c, uint32_t from) {
  const double est = (double)c * T.inv_w;
  uint32_t q = est < (double)(T.P - 1u) ? (uint32_t)est : T.P - 1u;
  if (q < from) q = from;
  while (q > from && T.E[q] > c) --q;
  while (q + 1u < T.P && T.E[q + 1u] <= c) ++q;
  return q;
}

// the interval [c0, c1) of context ctx, p0 = bin(c0); returns bin(c1)
__device__ __forceinline__ uint32_t epoch_add(EpochTab &T, uint32_t ctx, unsigned long long c0, unsigned long long c1,
                                              uint32_t p0, bool mid) {
  const uint32_t p1 = epoch_bin(T, c1, p0);
  if (p1 == p0) {
    atomicAdd(&T.part[p0 * 8u + ctx], c1 - c0);
  } else {
    atomicAdd(&T.part[p0 * 8u + ctx], T.E[p0 + 1u] - c0);
    atomicAdd(&T.part[p1 * 8u + ctx], c1 - T.E[p1]);
    if (p1 > p0 + 1u) {
      atomicAdd(&T.cov[(p0 + 1u) * 8u + ctx], 1);
      atomicAdd(&T.cov[p1 * 8u + ctx], -1);
    }
  }
  if (mid) atomicAdd(&T.J[p1 * 8u + ctx], 1u);
  return p1;
}

// The epoch walk of one triple: merge3's order and tie rules (left only if strictly below min(mid, right),
// else mid only if strictly below right, else right), every interval with the integer the whole-genome
// statistics add for it.
__device__ __forceinline__ void epoch_walk(const PathRef &L, const PathRef &M, const PathRef &R, uint64_t n,
                                           double tot_time, double scale, uint32_t p_start, EpochTab &T) {
  uint32_t ctx = 4u * L.init + 2u * M.init + R.init;
  double prev = 0.0;
  unsigned long long c = 0ull;
  uint32_t p = p_start;
  uint32_t i = 0, j = 0, k = 0;
  double tl = L.nj ? L.j[0] : EPV_INF;
  double tm = M.nj ? M.j[0] : EPV_INF;
  double tr = R.nj ? R.j[0] : EPV_INF;
  while (i < L.nj || j < M.nj || k < R.nj) {
    if (tl < (tm < tr ? tm : tr)) {
      const unsigned long long c1 = c + epv_stat_fix(tl - prev, scale);
      p = epoch_add(T, ctx, c, c1, p, false);
      c = c1; prev = tl; ctx ^= 4u; ++i;
      tl = i < L.nj ? L.j[(uint64_t)i * n] : EPV_INF;
    } else if (tm < tr) {
      const unsigned long long c1 = c + epv_stat_fix(tm - prev, scale);
      p = epoch_add(T, ctx, c, c1, p, true);
      c = c1; prev = tm; ctx ^= 2u; ++j;
      tm = j < M.nj ? M.j[(uint64_t)j * n] : EPV_INF;
    } else {
      const unsigned long long c1 = c + epv_stat_fix(tr - prev, scale);
      p = epoch_add(T, ctx, c, c1, p, false);
      c = c1; prev = tr; ctx ^= 1u; ++k;
      tr = k < R.nj ? R.j[(uint64_t)k * n] : EPV_INF;
    }
  }
  (void)epoch_add(T, ctx, c, c + epv_stat_fix(tot_time - prev, scale), p, false);
}

// first .. last: the owned local sites (tiles start at `first`); tiles: 256-site tiles per block
// (1 .. EPV_EPOCH_MAX_TILES); acc[B][P][32].  Dynamic shared memory: 136 P bytes.
__global__ __launch_bounds__(256) void epv_epoch_accum_kernel(EpvDev S, uint64_t first, uint64_t last,
                                                              const double *statscale, uint32_t P, uint32_t tiles,
                                                              unsigned long long *acc) {
  extern __shared__ unsigned long long s_dyn[];
  unsigned long long *s_part = s_dyn;                  // [P][8]
  unsigned long long *s_E = s_dyn + (size_t)P * 8u;    // [P]
  uint32_t *s_J = (uint32_t *)(s_E + P);               // [P][8]
  int *s_cov = (int *)(s_J + (size_t)P * 8u);          // [P][8]
  __shared__ uint32_t s_cnt[8];       // triples without a jump, per context
  __shared__ epv_meta_t s_meta[258];
  __shared__ uint8_t s_sel[258];
  // queue of the triples that need a walk: site offset in the block | the three sel bits << 13, and the
  // triple's three meta words
  __shared__ uint32_t s_ring[EPV_EPOCH_RING], s_ring_lm[EPV_EPOCH_RING];
  __shared__ epv_meta_t s_ring_r[EPV_EPOCH_RING];
  __shared__ uint32_t s_tail;
  const uint32_t t = threadIdx.x;
  const int lane = epv_lane();
  const uint32_t B = S.B, b = blockIdx.y;
  const uint64_t n = S.n, Bn = (uint64_t)B * n, Cn = (uint64_t)S.C * n;
  const uint64_t base0 = first + (uint64_t)blockIdx.x * tiles * 256u;
  const double scale = statscale[b + 1u], T_b = S.blen[b + 1u];
  const unsigned long long fixT = epv_stat_fix(T_b - 0.0, scale);

  for (uint32_t i = t; i < P * 8u; i += 256u) { s_part[i] = 0ull; s_J[i] = 0u; s_cov[i] = 0; }
  for (uint32_t p = t; p < P; p += 256u) s_E[p] = (unsigned long long)p * fixT / P;   // p fixT < 2^58
  if (t < 8u) s_cnt[t] = 0u;
  if (t == 0) s_tail = 0u;
  EpochTab T;
  T.part = s_part; T.J = s_J; T.cov = s_cov; T.E = s_E; T.P = P;
  T.inv_w = fixT ? (double)P / (double)fixT : 0.0;
  __syncthreads();
  const uint32_t p_zero = epoch_bin(T, 0ull, 0u);      // bin(0): 0 unless leading bins have no width

  auto walk_item = [&](uint32_t slot) __attribute__((always_inline)) {
    const uint32_t item = s_ring[slot], lm = s_ring_lm[slot], mr = s_ring_r[slot];
    const uint64_t si = base0 + (item & 0x1fffu);
    const uint32_t ml = lm & 0xffffu, mm = lm >> 16;
    PathRef L, M, R;
    L.j = S.jumps + ((item & (1u << 13)) ? Bn * S.C : 0ull) + (uint64_t)b * Cn + (si - 1); L.nj = ml & EPV_NJ_MASK; L.init = ml >> EPV_INIT_SHIFT;
    M.j = S.jumps + ((item & (1u << 14)) ? Bn * S.C : 0ull) + (uint64_t)b * Cn + si; M.nj = mm & EPV_NJ_MASK; M.init = mm >> EPV_INIT_SHIFT;
    R.j = S.jumps + ((item & (1u << 15)) ? Bn * S.C : 0ull) + (uint64_t)b * Cn + (si + 1); R.nj = mr & EPV_NJ_MASK; R.init = mr >> EPV_INIT_SHIFT;
    epoch_walk(L, M, R, n, T_b, scale, p_zero, T);
  };

  uint32_t head = 0u;
  // the sel byte of the next tile is fetched while this one is worked on (sel -> meta is a chain)
  uint64_t site = base0 + t;
  uint32_t my_sel = site < n ? S.sel[site] : 0u;
  for (uint32_t tile = 0; tile < tiles; ++tile) {
    const uint64_t site0 = base0 + (uint64_t)tile * 256u;
    if (site0 > last) break;                           // (block-uniform)
    site = site0 + t;
    const bool on = site <= last && site >= 1 && site + 1 < n;
    const bool edge = (t == 0 && site0 >= 1) || (t == 1 && site0 + 256u < n);
    const uint64_t esite = t == 0 ? site0 - 1 : site0 + 256u;
    const uint32_t e_sel = edge ? S.sel[esite] : 0u;
    const uint32_t m = site < n ? S.meta[(my_sel ? Bn : 0ull) + (uint64_t)b * n + site] : 0u;
    const uint32_t e_m = edge ? S.meta[(e_sel ? Bn : 0ull) + (uint64_t)b * n + esite] : 0u;
    const uint32_t cur_sel = my_sel;
    if (tile + 1u < tiles && site + 256u < n) my_sel = S.sel[site + 256u];
    s_meta[t + 1u] = (epv_meta_t)m;
    s_sel[t + 1u] = (uint8_t)cur_sel;
    if (t < 2u) {
      s_meta[t == 0 ? 0 : 257] = (epv_meta_t)e_m;
      s_sel[t == 0 ? 0 : 257] = (uint8_t)e_sel;
    }
    __syncthreads();
    const uint32_t ml = s_meta[t], mr = s_meta[t + 2u];
    const uint32_t sl = s_sel[t], sr = s_sel[t + 2u];
    const uint32_t or3 = (ml | m | mr) & EPV_NJ_MASK;
    const bool fast = on && or3 == 0u, slow = on && or3 != 0u;
    const unsigned long long mf = __ballot(fast), m2 = __ballot((ml >> EPV_INIT_SHIFT) != 0u),
                             m1 = __ballot((m >> EPV_INIT_SHIFT) != 0u), m0 = __ballot((mr >> EPV_INIT_SHIFT) != 0u);
    if (lane < 8) {
      const unsigned long long x = mf & ((lane & 4) ? m2 : ~m2) & ((lane & 2) ? m1 : ~m1) & ((lane & 1) ? m0 : ~m0);
      const uint32_t cnt = (uint32_t)__popcll(x);
      if (cnt) atomicAdd(&s_cnt[lane], cnt);
    }
    const unsigned long long ms = __ballot(slow);
    if (ms) {
      uint32_t base = 0u;
      if (lane == 0) base = atomicAdd(&s_tail, (uint32_t)__popcll(ms));
      base = epv_bcast(base, 0);
      if (slow) {
        const uint32_t slot = (base + (uint32_t)__popcll(ms & ((1ull << lane) - 1ull))) & (EPV_EPOCH_RING - 1u);
        s_ring[slot] = (tile * 256u + t) | ((sl ? 1u : 0u) << 13) | ((cur_sel ? 1u : 0u) << 14) | ((sr ? 1u : 0u) << 15);
        s_ring_lm[slot] = ml | (m << 16);
        s_ring_r[slot] = (epv_meta_t)mr;
      }
    }
    __syncthreads();
    // s_tail is only written again behind the next iteration's barrier; at most 255 + 256 items wait
    if (s_tail - head >= 256u) {
      walk_item((head + t) & (EPV_EPOCH_RING - 1u));
      head += 256u;
    }
  }
  __syncthreads();
  if (t < s_tail - head) walk_item((head + t) & (EPV_EPOCH_RING - 1u));
  // the triples without a jump: count x the one interval [0, fixT), whose bins are bin(0) and P - 1
  if (t < 8u) {
    const unsigned long long cnt = s_cnt[t];
    if (cnt) {
      const uint32_t pl = P - 1u;
      if (p_zero == pl) {
        atomicAdd(&s_part[pl * 8u + t], cnt * fixT);
      } else {
        atomicAdd(&s_part[p_zero * 8u + t], cnt * s_E[p_zero + 1u]);
        atomicAdd(&s_part[pl * 8u + t], cnt * (fixT - s_E[pl]));
        if (pl > p_zero + 1u) {
          atomicAdd(&s_cov[(p_zero + 1u) * 8u + t], (int)cnt);
          atomicAdd(&s_cov[pl * 8u + t], -(int)cnt);
        }
      }
    }
  }
  __syncthreads();
  unsigned long long *row = acc + (uint64_t)b * P * 32u;
  for (uint32_t i = t; i < P * 8u; i += 256u) {
    unsigned long long *cell = row + (uint64_t)(i >> 3) * 32u + (i & 7u);
    const uint32_t vj = s_J[i];
    const unsigned long long vp = s_part[i];
    const int vc = s_cov[i];
    if (vj) atomicAdd(cell, (unsigned long long)vj);
    if (vp & 0xffffffffull) atomicAdd(cell + 8, vp & 0xffffffffull);
    if (vp >> 32) atomicAdd(cell + 16, vp >> 32);
    if (vc) atomicAdd(cell + 24, (unsigned long long)(long long)vc);
  }
}

#endif
