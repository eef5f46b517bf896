// epv_epochs.cpp -- see epv_epochs.hpp
#include "epv_epochs.hpp"

#include <cmath>
#include <stdexcept>

namespace epv {

void epoch_edges(uint64_t fixT, uint32_t P, uint64_t *out) {
  for (uint32_t p = 0; p < P; ++p) out[p] = (uint64_t)((unsigned __int128)p * fixT / P);
}

void epoch_close(const uint64_t *raw, const uint64_t *fixT, uint32_t B, uint32_t P, uint64_t *closed) {
  for (uint32_t b = 0; b < B; ++b) {
    __int128 run[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // prefix sums of cov
    for (uint32_t p = 0; p < P; ++p) {
      const uint64_t *r = raw + ((uint64_t)b * P + p) * 32u;
      uint64_t *o = closed + ((uint64_t)b * P + p) * 24u;
      const uint64_t e0 = (uint64_t)((unsigned __int128)p * fixT[b] / P);
      const uint64_t e1 = p + 1u < P ? (uint64_t)((unsigned __int128)(p + 1u) * fixT[b] / P) : e0;
      for (int c = 0; c < 8; ++c) {
        o[c] = r[c];
        run[c] += (int64_t)r[24 + c];
        if (run[c] < 0) throw std::runtime_error("epoch_close: a negative cover count (not an accumulator's raw part)");
        if (p + 1u == P && run[c] != 0) throw std::runtime_error("epoch_close: the last epoch is covered wholly");
        const unsigned __int128 d = (unsigned __int128)r[8 + c] + ((unsigned __int128)r[16 + c] << 32) +
                                    (unsigned __int128)(e1 - e0) * (unsigned __int128)run[c];
        o[8 + c] = (uint64_t)d;
        o[16 + c] = (uint64_t)(d >> 64);
      }
    }
  }
}

void epoch_counts_to_stats(const uint64_t *closed, const int *k, uint32_t B, uint32_t P, uint64_t samples, double *J,
                           double *D) {
  if (!samples) throw std::runtime_error("epoch_counts_to_stats: no sample");
  const double ns = (double)samples;
  for (uint32_t b = 0; b < B; ++b) {
    const double inv = std::ldexp(1.0, -k[b]);     // a power of two: exact
    for (uint32_t p = 0; p < P; ++p) {
      const uint64_t *o = closed + ((uint64_t)b * P + p) * 24u;
      for (int c = 0; c < 8; ++c) {
        const unsigned __int128 d = (unsigned __int128)o[8 + c] | ((unsigned __int128)o[16 + c] << 64);
        J[((uint64_t)b * P + p) * 8u + c] = (double)(int64_t)o[c] / ns;
        D[((uint64_t)b * P + p) * 8u + c] = (double)d * inv / ns;
      }
    }
  }
}

}  // namespace epv
