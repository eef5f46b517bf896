// epv_origin.h -- lineage origin maps: on which branch the state a leaf shows at a site arose, and how long
// it has been held, counted over the sampled histories.  The lineage of leaf l is v_0 = l, v_1 = parent(v_0),
// ..., v_{d-1} (the child of the root).  A sample finds i* = the first i with a jump on branch v_i (k >= 1 in
// the 16-bit meta word) and adds
//   origin[row(l, i*)][s] += 1,   age[l][s] += sum_{i < i*} fixT[v_i] + fix(T_{v_i*} - t_last)
// where t_last is the LAST jump of branch v_i* (the only jump time read); without a jump on the lineage it
// adds to the leaf's root row d and age += sum_{i < d} fixT[v_i] (censored at the leaf's depth).
// fixT[v] = llrint(ldexp(T_v, k)) comes from the host, fix(x) = epv_stat_fix(x, 2^k) is one fp64 subtract,
// one multiply, round to nearest even; everything else is integer, so the result depends on no launch shape.
// Accumulators: origin uint32 [R][cnt], age uint64 [L][cnt] (sites fastest) over the sites a context counts.
// Every cell has one owner thread: plain loads and stores, no atomics.  No LDS.
#ifndef EPV_ORIGIN_H
#define EPV_ORIGIN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"
#include "epv_kernels.h"

#define EPV_ORG_CH 4u   /* lineage branches whose meta loads are in flight together */

// blockIdx.y = leaf, one thread per site of lo .. lo + cnt - 1.  first[l] .. first[l + 1] - 1 are the rows of
// leaf l; rowb[r] = the branch node of row r (0 = the root row, a leaf's last), so rowb[first[l] ..] IS the
// lineage: the walk needs no parent chase.  The leaf, its rows and fixT are uniform over the block (scalar
// loads); a wave's meta loads of one branch are unit-stride, and the ancestors' words, which every leaf
// below them reads again, come from cache.  Per site and leaf: one origin cell and one age cell written.
__global__ __launch_bounds__(256) void epv_origin_accum_kernel(EpvDev S, uint64_t lo, uint64_t cnt,
                                                               const uint32_t *first, const uint32_t *rowb,
                                                               const long long *fixT, double scale,
                                                               uint32_t *origin, unsigned long long *age) {
  const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (s >= cnt) return;
  const uint32_t leaf = blockIdx.y;
  const uint64_t site = lo + s, n = S.n;
  const uint32_t buf = S.sel[site];
  const epv_meta_t *m = S.meta + (buf ? (uint64_t)S.B * n : 0ull) + site;
  const uint32_t r0 = first[leaf], r1 = first[leaf + 1u] - 1u;   // r1: the root row
  unsigned long long held = 0;   // fixT of the jump-free branches below the origin
  uint32_t row = r1;
  for (uint32_t r = r0; r < r1; r += EPV_ORG_CH) {
    // no branch between the loads: a row index beyond the lineage is clamped to the root row (rowb = 0), and
    // a node 0 reads branch 0's word (in bounds), which is masked away afterwards
    uint32_t v[EPV_ORG_CH], w[EPV_ORG_CH];
#pragma unroll
    for (uint32_t i = 0; i < EPV_ORG_CH; ++i) v[i] = rowb[r + i < r1 ? r + i : r1];
#pragma unroll
    for (uint32_t i = 0; i < EPV_ORG_CH; ++i) w[i] = (uint32_t)m[(uint64_t)(v[i] ? v[i] - 1u : 0u) * n];
#pragma unroll
    for (uint32_t i = 0; i < EPV_ORG_CH; ++i) w[i] = v[i] ? w[i] : 0u;
    bool found = false;
#pragma unroll
    for (uint32_t i = 0; i < EPV_ORG_CH; ++i) {
      if (found || r + i >= r1) continue;
      const uint32_t k = w[i] & EPV_NJ_MASK;
      if (!k) {
        held += (unsigned long long)fixT[v[i]];
        continue;
      }
      const uint64_t b = v[i] - 1u;
      const double t_last = S.jumps[(((buf ? (uint64_t)S.B : 0ull) + b) * S.C + (k - 1u)) * n + site];
      held += epv_stat_fix(S.blen[v[i]] - t_last, scale);
      row = r + i;
      found = true;
    }
    if (found) break;
  }
  origin[(uint64_t)row * cnt + s] += 1u;
  age[(uint64_t)leaf * cnt + s] += held;
}

#endif
