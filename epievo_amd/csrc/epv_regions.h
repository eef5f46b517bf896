// epv_regions.h -- fixed sites (epv_set_fixed_sites): the guards around a colour phase
// and the correction of the integer statistics.  Included by epv_abi.hip after epv_kernels.h.
//
// A fixed site is held by GUARDS around the untouched colour-phase kernels, not by a test inside them.  A phase
// of colour c writes, for a site s of that colour, the proposal into the buffer sel[s] ^ 1 (dead data until a
// flip) and, on acceptance, sel[s] and tri[s - 1 .. s + 1]; no other site of the colour (s +- 3, ...) writes
// or reads those three tri entries within the phase.  So saving (sel[s], tri[s - 1], tri[s], tri[s + 1]) of every
// fixed site of the colour before the phase and putting them back after it leaves the site, its cached
// likelihoods and the buffer its path lives in exactly as they were, whichever kernel family ran the phase.
// The lists hold local sites 1 .. n - 2 only (the two end columns of a context are never updated), so s - 1 and
// s + 1 are in range.  One lane per fixed site; the lists are tiny (two sites per region break).
//
// The accept counter.  The kernels count an acceptance in two places, and the guard takes both back:
//   * the acceptance stage flips sel[s] and counts: the restore kernel sees the flip;
//   * the second and third proposal kernel and the fused phase count a proposal EQUAL to the current path at once
//     ("accepted with probability one", epv_propose2.h step 5) and write nothing -- no flip to see.  Every other
//     proposal of theirs writes the start states of all branches into the other buffer's meta words.  So where
//     such a kernel runs the phase (ident_counts) the save kernel plants a mark in the other buffer's meta word of
//     branch 0 -- EPV_FIXED_MARK, a jump count no path can have -- keeping the word it replaces; a mark that is
//     still there after the phase means "equal proposal, counted" if the phase ran the site (first <= s <= last),
//     and the restore kernel puts the old word back.  The other buffer is dead data until a flip, which the
//     guard undoes, so nothing reads the mark.
#pragma once

#define EPV_FIXED_MARK ((epv_meta_t)EPV_NJ_MASK)   // 32767 jumps: above EPV_MAX_CAP, and no start state alone

// what the guard keeps of a fixed site over a phase: [site slot] words of `sel`, [3][site slot] doubles of `tri`
struct EpvFixedSave {
  uint32_t *sel;   // sel | the other buffer's meta word of branch 0 << 8 (kept under ident_counts)
  double *tri;   // tri[k * cap + i] = S.tri[site_i - 1 + k]
  uint64_t cap;
};

__global__ __launch_bounds__(64) void epv_fixed_save_kernel(EpvDev S, const uint64_t *sites, uint64_t count,
                                                            EpvFixedSave K, uint32_t ident_counts) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint64_t s = sites[i];
  const uint32_t sel = S.sel[s];
  uint32_t word = sel;
  if (ident_counts) {
    const uint64_t at = meta_idx(S, sel ^ 1u, 0u, s);
    word |= (uint32_t)S.meta[at] << 8;
    S.meta[at] = EPV_FIXED_MARK;
  }
  K.sel[i] = word;
  K.tri[i] = S.tri[s - 1];
  K.tri[K.cap + i] = S.tri[s];
  K.tri[2u * K.cap + i] = S.tri[s + 1];
}

// puts back what epv_fixed_save_kernel kept.  A site whose sel bit differs, or whose mark is still there (above),
// was counted as accepted by the phase if it lies in the owned range: it is taken off the accept counter again
// (the counter is kept in shards that are summed modulo 2^64: subtracting from shard 0 is exact whatever shard
// counted it).  first, last: the range of sites the phase ran
__global__ __launch_bounds__(64) void epv_fixed_restore_kernel(EpvDev S, const uint64_t *sites, uint64_t count,
                                                               EpvFixedSave K, uint64_t first, uint64_t last,
                                                               uint64_t own_first, uint64_t own_last,
                                                               uint32_t ident_counts, unsigned long long *counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool undone = false;
  if (i < count) {
    const uint64_t s = sites[i];
    const uint32_t word = K.sel[i], sel = word & 1u;
    bool counted = S.sel[s] != sel;
    if (ident_counts) {
      const uint64_t at = meta_idx(S, sel ^ 1u, 0u, s);
      if (S.meta[at] == EPV_FIXED_MARK) {
        S.meta[at] = (epv_meta_t)(word >> 8);
        counted = s >= first && s <= last;
      }
    }
    undone = counted && s >= own_first && s <= own_last;
    S.sel[s] = (uint8_t)sel;
    S.tri[s - 1] = K.tri[i];
    S.tri[s] = K.tri[K.cap + i];
    S.tri[s + 1] = K.tri[2u * K.cap + i];
  }
  const unsigned long long um = __ballot(undone);
  if (um && epv_lane() == 0)
    atomicAdd(&counters[EPV_CNT_IDX(EPV_CNT_ACCEPT, 0u)], 0ull - (unsigned long long)__popcll(um));
}

// ---- statistics.  The statistics kernels count the triple of every centre of the owned range; a fixed site is no
// centre.  One lane per (fixed site, branch) computes that triple's events exactly as the statistics kernels do
// (merge3, epv_stat_fix) and SUBTRACTS them from the 16 integer words of the branch at `tot` ([B][16], J then D).
// Integer sums commute modulo 2^64, so what is left is "all centres minus the fixed ones" to the bit, wherever in
// the reduction `tot` sits: a finished row of d_sweep_tot, or a row of the wave kernel's partial sums.
struct AccExactSub {
  unsigned long long *acc;
  double scale;
};
__device__ __forceinline__ void acc_add(AccExactSub &A, int ctx, double dt, bool mid) {
  atomicAdd(&A.acc[8 + ctx], 0ull - epv_stat_fix(dt, A.scale));
  if (mid) atomicAdd(&A.acc[ctx], 0ull - 1ull);
}

__global__ __launch_bounds__(64) void epv_fixed_unstat_kernel(EpvDev S, const uint64_t *sites, uint64_t count,
                                                              uint64_t first, uint64_t last, const double *statscale,
                                                              unsigned long long *tot) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t B = S.B;
  if (t >= count * B) return;
  const uint64_t s = sites[t / B];
  const uint32_t b = (uint32_t)(t % B);
  if (s < first || s > last) return;   // (the lists hold 1 .. n - 2 only)
  const PathRef L = path_ref(S, S.sel[s - 1], b, s - 1), M = path_ref(S, S.sel[s], b, s),
                R = path_ref(S, S.sel[s + 1], b, s + 1);
  AccExactSub A;
  A.acc = tot + (uint64_t)b * 16u;
  A.scale = statscale[b + 1u];
  merge3(L, M, R, S.n, S.blen[b + 1u], A);
}
