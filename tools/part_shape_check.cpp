// part_shape_check.cpp -- a stand-alone check of epievo_amd/csrc/epv_part.h, the one place that computes the byte
// sizes of the parts of the five summaries that are joint along the genome.  Every size is compared with the
// expression the layer's alloc, reset and get functions each wrote out by hand before there was a part shape (below,
// in plain numbers: 128 bins, 27 tract classes), over N in {2, 5, 31}, cnt in {0, 1, 64, 65}, max in {1, 2^21} and a
// few lags and sizes; some values are pinned as numbers worked out by hand.  No GPU, no HIP:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I epievo_amd/csrc
//       -o part_shape_check tools/part_shape_check.cpp && ./part_shape_check
#include <cstdio>
#include <cstdlib>

#include "epv_part.h"

static int failures = 0;

static void same(const char *layer, const char *what, unsigned long long got, unsigned long long want, uint32_t N,
                 uint64_t cnt, uint64_t max) {
  if (got == want) return;
  ++failures;
  std::fprintf(stderr, "part_shape_check: %s %s = %llu, expected %llu (N %u, cnt %llu, max %llu)\n", layer, what, got, want,
               N, (unsigned long long)cnt, (unsigned long long)max);
}

// rows, words, scratch, one sample's edge records, all edge records, the two accumulators
struct Want {
  unsigned long long rows, words, bits_b, edge_b, edges_b, acc0_b, acc1_b;
};
static void check(const char *layer, const PartShape &s, const Want &w, uint32_t N, uint64_t cnt, uint64_t max) {
  same(layer, "rows", s.rows, w.rows, N, cnt, max);
  same(layer, "words", s.words, w.words, N, cnt, max);
  same(layer, "bits_b", s.bits_b, w.bits_b, N, cnt, max);
  same(layer, "edge_b", s.edge_b, w.edge_b, N, cnt, max);
  same(layer, "edges_b", s.edges_b, w.edges_b, N, cnt, max);
  same(layer, "acc_b[0]", s.acc_b[0], w.acc0_b, N, cnt, max);
  same(layer, "acc_b[1]", s.acc_b[1], w.acc1_b, N, cnt, max);
  same(layer, "total", s.total(), w.bits_b + w.edges_b + w.acc0_b + w.acc1_b, N, cnt, max);
}

int main() {
  const uint32_t Ns[] = {2u, 5u, 31u};
  const uint64_t cnts[] = {0u, 1u, 64u, 65u}, maxes[] = {1u, 1ull << 21};
  const uint32_t lags[] = {1u, 64u, 65u, 1024u};
  const uint32_t sizes[][2] = {{1u, 1u}, {2u, 20u}, {4u, 1024u}};   // K and the largest size
  for (const uint32_t N : Ns)
    for (const uint64_t cnt : cnts)
      for (const uint64_t max : maxes) {
        const unsigned long long B = N - 1u, n = N, words = (cnt + 63u) / 64u, R2 = 2u * B;
        check("domains", domains_shape(N, cnt, max),
              {n, words, 8u * n * words, 16u * n, 16u * n * max, 16u * 128u * n, 16u * n}, N, cnt, max);
        check("turnover", turnover_shape(N - 1u, cnt, max),
              {R2, words, 8u * R2 * words, 16u * R2, 16u * R2 * max, 32u * 128u * R2, 32u * R2}, N, cnt, max);
        check("tracts", tracts_shape(N - 1u, cnt, max),
              {R2, words, 16u * B * words, 16u * B, 16u * B * max, 8u * 27u * 128u * B, 8u * 27u * B}, N, cnt, max);
        for (const uint32_t L : lags) {
          const unsigned long long R = n + B, LW = (L + 63u) / 64u;
          check("corr", corr_shape(N, N - 1u, L, cnt, max),
                {R, words, 8u * R * words, 16u * R * LW, 16u * R * LW * max, 8u * R * (L + 1ull), 0u}, N, cnt, max);
        }
        for (const auto &z : sizes) {
          const unsigned long long K = z[0], E = 2u * (z[1] - 1u), EW = (E + 63u) / 64u;
          same("dmaps", "edge bits", dmaps_edge_bits(z[1]), E, N, cnt, max);
          check("dmaps", dmaps_shape(N, z[0], z[1], cnt, max),
                {n, words, 8u * n * words, 16u * n * EW, 16u * n * EW * max, 4u * n * K * cnt, 0u}, N, cnt, max);
        }
      }
  // by hand: the 5-node tree over 65 sites, 2 samples
  check("domains", domains_shape(5u, 65u, 2u), {5u, 2u, 80u, 80u, 160u, 10240u, 80u}, 5u, 65u, 2u);
  check("turnover", turnover_shape(4u, 65u, 2u), {8u, 2u, 128u, 128u, 256u, 32768u, 256u}, 5u, 65u, 2u);
  check("tracts", tracts_shape(4u, 65u, 2u), {8u, 2u, 128u, 64u, 128u, 110592u, 864u}, 5u, 65u, 2u);
  check("corr", corr_shape(5u, 4u, 65u, 65u, 2u), {9u, 2u, 144u, 288u, 576u, 4752u, 0u}, 5u, 65u, 2u);
  check("dmaps", dmaps_shape(5u, 2u, 20u, 65u, 2u), {5u, 2u, 80u, 80u, 160u, 2600u, 0u}, 5u, 65u, 2u);
  if (failures) return EXIT_FAILURE;
  std::puts("part_shape_check: every size as written out before");
  return EXIT_SUCCESS;
}
