// epv_pavg.h -- the average history of the sampled paths (average_paths.cpp:31-45 of the
// reference, on the device).  For P grid points t_0 = 0, t_{i+1} = t_i + bin, bin = T_b / (P - 1)
// (repeated fp64 addition, as the reference does it), the value of a path at point i >= 1 is
// Path::state_at_time(t_i) = init XOR (parity of the jumps < t_i), at point 0 its init state.
//
// Accumulator: int32 [b][i][s] over the sites a context counts (sites fastest):
//   row 0       running count of init states (one coalesced read-modify-write per sweep)
//   rows i >= 1 difference counts: jump j at time tau goes to row k = min{i >= 1 : t_i > tau}
//               with +1 if the state before it was 0, -1 otherwise (nothing when no t_i > tau)
// so that count[i] = rows 0..i summed.  A (site, branch) without jumps costs the row-0 update only.
// Every (b, s) has one owner thread: plain loads and stores, no atomics.
#ifndef EPV_PAVG_H
#define EPV_PAVG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"

// grid[b * P + i] = t_i of branch b + 1 (uploaded by the host, built by the recurrence above)
__device__ __forceinline__ uint32_t epv_pavg_cell(const double *tg, uint32_t P, double tau) {
  // guess from the quotient, then correct against the table: the cut is the table's, bit for bit
  const double q = tau / tg[1];
  uint32_t g = q < (double)(P - 1u) ? (uint32_t)q + 1u : P;
  while (g > 1u && tg[g - 1u] > tau) --g;
  while (g < P && tg[g] <= tau) ++g;
  return g;   // P: no grid point lies above tau
}

// one thread per (site, branch) of sites lo .. lo + cnt - 1 (blockIdx.y = branch)
__global__ __launch_bounds__(256) void epv_pavg_accum_kernel(EpvDev S, uint64_t lo, uint64_t cnt,
                                                             const double *grid, uint32_t P, int32_t *acc) {
  const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (s >= cnt) return;
  const uint32_t b = blockIdx.y;
  const uint64_t site = lo + s, n = S.n;
  const uint32_t buf = S.sel[site];
  const uint32_t m = S.meta[(buf ? (uint64_t)S.B * n : 0ull) + (uint64_t)b * n + site];
  const uint32_t nj = m & EPV_NJ_MASK;
  uint32_t state = m >> EPV_INIT_SHIFT;
  int32_t *a = acc + (uint64_t)b * P * cnt + s;
  a[0] += (int32_t)state;
  if (!nj) return;
  const double *j = S.jumps + (buf ? (uint64_t)S.B * S.C * n : 0ull) + (uint64_t)b * S.C * n + site;
  const double *tg = grid + (uint64_t)b * P;
  // jumps ascend, so their cells do too: the deltas of one cell are combined before the write
  uint32_t cell = P;
  int32_t delta = 0;
  for (uint32_t k = 0; k < nj; ++k) {
    const uint32_t c = epv_pavg_cell(tg, P, j[(uint64_t)k * n]);
    if (c == P) break;
    const int32_t d = state ? -1 : 1;
    state ^= 1u;
    if (c != cell) {
      if (cell < P && delta) a[(uint64_t)cell * cnt] += delta;
      cell = c;
      delta = d;
    } else {
      delta += d;
    }
  }
  if (cell < P && delta) a[(uint64_t)cell * cnt] += delta;
}

// read-out: count[b][s][i] = rows 0..i summed, for sites first .. first + count - 1 of the
// accumulator (relative to its first site), transposed through LDS.  64 sites of one branch per
// block; points in chunks of 64.  The accumulator is only read.
#define EPV_PAVG_RD 64u
__global__ __launch_bounds__(64) void epv_pavg_read_kernel(const int32_t *acc, uint32_t P, uint64_t cnt,
                                                           uint64_t first, uint64_t count, uint32_t *out) {
  __shared__ uint32_t tile[EPV_PAVG_RD][EPV_PAVG_RD + 1u];
  const uint32_t t = threadIdx.x, b = blockIdx.y;
  const uint64_t s0 = (uint64_t)blockIdx.x * EPV_PAVG_RD, s = s0 + t;
  const bool on = s < count;
  const int32_t *a = acc + (uint64_t)b * P * cnt + first + s;
  uint32_t *o = out + ((uint64_t)b * count + s0) * P;
  const uint32_t rows = count - s0 < EPV_PAVG_RD ? (uint32_t)(count - s0) : EPV_PAVG_RD;
  int32_t run = 0;
  for (uint32_t i0 = 0; i0 < P; i0 += EPV_PAVG_RD) {
    const uint32_t w = P - i0 < EPV_PAVG_RD ? P - i0 : EPV_PAVG_RD;
    if (on)
      for (uint32_t i = 0; i < w; ++i) {
        run += a[(uint64_t)(i0 + i) * cnt];
        tile[t][i] = (uint32_t)run;
      }
    __syncthreads();
    if (t < w)
      for (uint32_t r = 0; r < rows; ++r) o[(uint64_t)r * P + i0 + t] = tile[r][t];
    __syncthreads();
  }
}

#endif
