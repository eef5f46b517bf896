// epv_bevents.h -- posterior branch-event maps: what happened on branch b at site s, counted over the
// sampled histories.  A sample needs the 16-bit meta word alone: a = init state, k = number of jumps
// (no jump time is read).  With e = a XOR (k & 1) the end state, g = (k + (a == 0)) >> 1 the 0->1 jumps
// and l = k - g the 1->0 jumps, a sample adds to six uint32 planes [plane][b][s] (sites fastest) over
// the sites a context counts:
//   0 end1      e                     1 net_gain  a == 0 && e == 1      2 net_loss  a == 1 && e == 0
//   3 changed   k >= 1                4 gains     g                     5 losses    l
// A path holds at most EPV_MAX_CAP = 2047 jumps, so g, l <= 1024 and EPV_BEV_MAX_SAMPLES = 2^21 samples
// stay below 2^32 in every cell.  Every cell has one owner thread: plain loads and stores, no atomics.
#ifndef EPV_BEVENTS_H
#define EPV_BEVENTS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "epv_device.h"

#define EPV_BEV_PLANES 6u
#define EPV_BEV_MAX_SAMPLES (1ull << 21)
#define EPV_BEV_BCH 8u   /* branches whose meta loads are in flight together */

// one thread per site of lo .. lo + cnt - 1: sel once, then the current buffer's meta words of all
// branches, EPV_BEV_BCH loads at a time.  A plane is read-modified-written only where its increment is
// not zero: the common pair (k = 0) touches plane 0 when a = 1 and nothing when a = 0.
__global__ __launch_bounds__(256) void epv_bevents_accum_kernel(EpvDev S, uint64_t lo, uint64_t cnt, uint32_t *acc) {
  const uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (s >= cnt) return;
  const uint64_t site = lo + s, n = S.n;
  const uint32_t B = S.B;
  const epv_meta_t *m = S.meta + (S.sel[site] ? (uint64_t)B * n : 0ull) + site;
  const uint64_t plane = (uint64_t)B * cnt;
  for (uint32_t b0 = 0; b0 < B; b0 += EPV_BEV_BCH) {
    uint32_t w[EPV_BEV_BCH];
#pragma unroll
    for (uint32_t i = 0; i < EPV_BEV_BCH; ++i)   // (a = 0, k = 0 beyond the last branch: nothing to add)
      w[i] = b0 + i < B ? (uint32_t)m[(uint64_t)(b0 + i) * n] : 0u;
#pragma unroll
    for (uint32_t i = 0; i < EPV_BEV_BCH; ++i) {
      if (!w[i]) continue;
      const uint32_t a = w[i] >> EPV_INIT_SHIFT, k = w[i] & EPV_NJ_MASK;
      uint32_t *c = acc + (uint64_t)(b0 + i) * cnt + s;
      if (a ^ (k & 1u)) c[0] += 1u;
      if (!k) continue;
      if (k & 1u) c[(a ? 2u : 1u) * plane] += 1u;
      c[3u * plane] += 1u;
      const uint32_t g = (k + (a ^ 1u)) >> 1, l = k - g;
      if (g) c[4u * plane] += g;
      if (l) c[5u * plane] += l;
    }
  }
}

// window read-out: out[p][b][w - w0] (uint64) = plane p of branch b summed over the counted sites that
// lie in window w = global sites [w W, (w + 1) W), for windows w0 .. w0 + nw - 1; zero where the
// context counts no site of a window.  The counted sites are global glo .. glo + cnt - 1.  A block of
// 256 threads serves 256 / Wp windows of one (plane, branch) row, Wp = the power of two >= W up to 64, else 256:
// the lanes of a window read its sites in steps of Wp (adjacent windows are adjacent in memory, so a
// wave's loads are contiguous), then a butterfly over the Wp lanes in integers -- within the wave by
// shuffles, across the four waves (Wp = 256) through LDS.  Integer sums: the result depends on no
// launch shape.  W <= n_global (the host clamps it).  The accumulator is only read.
__global__ __launch_bounds__(256) void epv_bevents_window_kernel(const uint32_t *acc, uint32_t B, uint64_t cnt,
                                                                 uint64_t glo, uint64_t n_global, uint64_t W,
                                                                 uint32_t Wp, uint64_t w0, uint64_t nw,
                                                                 unsigned long long *out) {
  __shared__ unsigned long long part[4];
  const uint32_t t = threadIdx.x, row = blockIdx.y;   // row = plane * B + branch
  const uint32_t per_block = 256u / Wp, j0 = t % Wp;
  const uint64_t wi = (uint64_t)blockIdx.x * per_block + t / Wp;   // window of this lane, relative to w0
  const uint64_t n_win = (n_global + W - 1u) / W;
  unsigned long long sum = 0;
  if (wi < nw && w0 + wi < n_win) {
    const uint64_t g0 = (w0 + wi) * W;
    const uint64_t g1 = n_global - g0 < W ? n_global : g0 + W;
    const uint64_t a = g0 > glo ? g0 : glo, e = g1 < glo + cnt ? g1 : glo + cnt;
    const uint32_t *p = acc + (uint64_t)row * cnt;
    uint64_t g = g0 + j0;
    if (g < a) g += (a - g + Wp - 1u) / Wp * Wp;   // this lane's first counted site
    for (; g < e; g += Wp) sum += p[g - glo];
  }
  const uint32_t in_wave = Wp < 64u ? Wp : 64u;
  for (uint32_t d = 1; d < in_wave; d <<= 1) sum += __shfl_xor(sum, (int)d, 64);
  if (Wp == 256u) {
    if ((t & 63u) == 0u) part[t >> 6] = sum;
    __syncthreads();
    sum = part[0] + part[1] + part[2] + part[3];
  }
  if (j0 == 0u && wi < nw) out[(uint64_t)row * nw + wi] = sum;
}

#endif
