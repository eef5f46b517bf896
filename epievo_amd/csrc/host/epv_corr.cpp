// epv_corr.cpp -- see epv_corr.hpp
#include "epv_corr.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace epv {

namespace {
// word j of the LW-word string x shifted right by sh bits (sh <= 64 LW); no shift by 64 is formed
inline uint64_t shr_word(const uint64_t *x, uint32_t LW, uint32_t sh, uint32_t j) {
  const uint32_t q = sh >> 6, s = sh & 63u;
  const uint64_t a = j + q < LW ? x[j + q] : 0u;
  if (!s) return a;
  const uint64_t b = j + q + 1u < LW ? x[j + q + 1u] : 0u;
  return (a >> s) | (b << (64u - s));
}
inline uint64_t bit_of(const uint64_t *x, uint32_t j) { return (x[j >> 6] >> (j & 63u)) & 1u; }

void check_dims(uint32_t L, const char *who) {
  if (L == 0u || L > kCorrMaxLag) throw std::runtime_error(std::string(who) + ": max_lag is 1 .. 1024");
}
}  // namespace

uint64_t corr_parts_merge(uint64_t n_parts, uint32_t R, uint32_t L, uint64_t samples, const uint64_t *cnts,
                          const uint64_t *const *n11s, const uint64_t *const *edges, uint64_t *out_n11,
                          uint64_t *out_edges) {
  check_dims(L, "corr_parts_merge");
  if (!n_parts) throw std::runtime_error("corr_parts_merge: no parts");
  const uint32_t LW = corr_edge_words(L);
  const uint64_t nn = (uint64_t)R * (L + 1u);
  uint64_t total = 0;
  for (uint64_t p = 0; p < n_parts; ++p) {
    if (cnts[p] < L)
      throw std::runtime_error("corr_parts_merge: part " + std::to_string(p) + " holds " + std::to_string(cnts[p]) +
                               " sites, fewer than max_lag = " + std::to_string(L) +
                               ": a pair would span three parts");
    total += cnts[p];
  }
  std::fill(out_n11, out_n11 + nn, 0u);
  for (uint64_t p = 0; p < n_parts; ++p)
    for (uint64_t i = 0; i < nn; ++i) out_n11[i] += n11s[p][i];
  for (uint64_t s = 0; s < samples; ++s)
    for (uint32_t r = 0; r < R; ++r) {
      const uint64_t at = (s * R + r) * 2u * LW;
      // a tail of L bits holds every site within L of the boundary: no earlier part reaches across it
      for (uint64_t p = 0; p + 1u < n_parts; ++p) {
        const uint64_t *tail = edges[p] + at + LW, *head = edges[p + 1u] + at;
        for (uint32_t d = 1; d <= L; ++d) {
          // tail >> (L - d) leaves its last d bits at 0 .. d - 1; the spare bits above are zero
          uint64_t c = 0;
          const uint32_t nw = (d + 63u) >> 6;
          for (uint32_t j = 0; j < nw; ++j) c += (uint64_t)__builtin_popcountll(shr_word(tail, LW, L - d, j) & head[j]);
          out_n11[(uint64_t)r * (L + 1u) + d] += c;
        }
      }
      std::copy(edges[0] + at, edges[0] + at + LW, out_edges + at);
      std::copy(edges[n_parts - 1u] + at + LW, edges[n_parts - 1u] + at + 2u * LW, out_edges + at + LW);
    }
  return total;
}

void corr_part_close(uint32_t R, uint32_t L, uint64_t samples, uint64_t n, const uint64_t *n11, const uint64_t *edges,
                     uint64_t *left1, uint64_t *right1) {
  check_dims(L, "corr_part_close");
  if (n < L)
    throw std::runtime_error("corr_part_close: the part holds " + std::to_string(n) + " sites, fewer than max_lag = " +
                             std::to_string(L));
  const uint32_t LW = corr_edge_words(L);
  for (uint32_t r = 0; r < R; ++r)
    for (uint32_t d = 0; d <= L; ++d) left1[(uint64_t)r * (L + 1u) + d] = right1[(uint64_t)r * (L + 1u) + d] = n11[(uint64_t)r * (L + 1u)];
  for (uint64_t s = 0; s < samples; ++s)
    for (uint32_t r = 0; r < R; ++r) {
      const uint64_t *head = edges + (s * R + r) * 2u * LW, *tail = head + LW;
      uint64_t in_head = 0, in_tail = 0;   // the ones among the first d and among the last d sites
      for (uint32_t d = 1; d <= L; ++d) {
        in_head += bit_of(head, d - 1u);
        in_tail += bit_of(tail, L - d);
        left1[(uint64_t)r * (L + 1u) + d] -= in_tail;
        right1[(uint64_t)r * (L + 1u) + d] -= in_head;
      }
    }
}

}  // namespace epv
