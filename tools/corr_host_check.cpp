// corr_host_check.cpp -- a stand-alone check of host/epv_corr.cpp, which indexes bit windows by hand: random 0/1 rows
// are cut into pieces of at least max_lag sites (one of exactly max_lag), the pieces' parts are merged and closed, and
// the result is compared with a count over the whole rows, pair by pair.  Meant to be built with the sanitizers and
// run on the CPU; it prints "ok" and returns 0, or says what differs.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I epievo_amd/csrc/host \
//       -o corr_host_check tools/corr_host_check.cpp epievo_amd/csrc/host/epv_corr.cpp && ./corr_host_check
#include <cstdint>
#include <cstdio>
#include <exception>
#include <random>
#include <vector>

#include "epv_corr.hpp"

namespace {
using Row = std::vector<uint8_t>;

struct Part {
  uint64_t cnt = 0;
  std::vector<uint64_t> n11, edges;   // exactly R (L + 1) and samples R 2 LW words: the sanitizer sees any overrun
};

// the part of samples x R rows over sites [a, b), by the definition
Part part_of(const std::vector<std::vector<Row>> &xs, uint32_t R, uint32_t L, uint64_t a, uint64_t b) {
  const uint32_t LW = epv::corr_edge_words(L);
  Part p;
  p.cnt = b - a;
  p.n11.assign((size_t)R * (L + 1u), 0u);
  p.edges.assign(xs.size() * R * 2u * LW, 0u);
  for (size_t s = 0; s < xs.size(); ++s)
    for (uint32_t r = 0; r < R; ++r) {
      const Row &x = xs[s][r];
      for (uint32_t d = 0; d <= L; ++d)
        for (uint64_t i = a; i + d < b; ++i) p.n11[(size_t)r * (L + 1u) + d] += x[i] & x[i + d];
      uint64_t *head = p.edges.data() + (s * R + r) * 2u * LW, *tail = head + LW;
      for (uint32_t j = 0; j < L; ++j) {
        head[j >> 6] |= (uint64_t)x[a + j] << (j & 63u);
        tail[j >> 6] |= (uint64_t)x[b - L + j] << (j & 63u);
      }
    }
  return p;
}

int fail(const char *what, uint32_t L, uint64_t n) {
  std::fprintf(stderr, "corr_host_check: %s (max_lag %u, %llu sites)\n", what, L, (unsigned long long)n);
  return 1;
}
}  // namespace

int main() {
  std::mt19937_64 rng(12345);
  const uint32_t lags[] = {1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024};
  for (uint32_t L : lags)
    for (int trial = 0; trial < (L > 200 ? 3 : 12); ++trial) {
      const uint32_t R = 1u + (uint32_t)(rng() % 3u), k = 1u + (uint32_t)(rng() % 4u);
      const uint64_t samples = 1u + rng() % 3u;
      // piece sizes: one of exactly L, the others L plus something
      std::vector<uint64_t> cuts(1, 0u);
      const uint32_t exact = (uint32_t)(rng() % k);
      for (uint32_t i = 0; i < k; ++i) cuts.push_back(cuts.back() + L + (i == exact ? 0u : rng() % (2u * L + 70u)));
      const uint64_t n = cuts.back();
      std::vector<std::vector<Row>> xs(samples, std::vector<Row>(R, Row(n, 0)));
      for (auto &sample : xs)
        for (Row &x : sample) {
          const unsigned kind = (unsigned)(rng() % 4u);
          for (uint64_t i = 0; i < n; ++i)
            x[i] = kind == 0 ? (uint8_t)(rng() & 1u) : kind == 1 ? 1 : kind == 2 ? (uint8_t)(rng() % 50u == 0) : (uint8_t)((i / 37u) & 1u);
        }
      std::vector<Part> parts;
      for (uint32_t i = 0; i < k; ++i) parts.push_back(part_of(xs, R, L, cuts[i], cuts[i + 1]));
      const Part whole = part_of(xs, R, L, 0, n);
      std::vector<uint64_t> cnts;
      std::vector<const uint64_t *> ap, ep;
      for (const Part &p : parts) { cnts.push_back(p.cnt); ap.push_back(p.n11.data()); ep.push_back(p.edges.data()); }
      Part got;
      got.n11.assign(whole.n11.size(), 7u);
      got.edges.assign(whole.edges.size(), 7u);
      got.cnt = epv::corr_parts_merge(k, R, L, samples, cnts.data(), ap.data(), ep.data(), got.n11.data(), got.edges.data());
      if (got.cnt != n || got.n11 != whole.n11 || got.edges != whole.edges) return fail("merge differs from the whole", L, n);
      if (k >= 2) {   // associative: the first piece, then the rest
        Part rest;
        rest.n11.assign(whole.n11.size(), 0u);
        rest.edges.assign(whole.edges.size(), 0u);
        rest.cnt = epv::corr_parts_merge(k - 1u, R, L, samples, cnts.data() + 1, ap.data() + 1, ep.data() + 1, rest.n11.data(),
                                         rest.edges.data());
        const uint64_t c2[2] = {cnts[0], rest.cnt};
        const uint64_t *a2[2] = {ap[0], rest.n11.data()}, *e2[2] = {ep[0], rest.edges.data()};
        Part two;
        two.n11.assign(whole.n11.size(), 0u);
        two.edges.assign(whole.edges.size(), 0u);
        two.cnt = epv::corr_parts_merge(2, R, L, samples, c2, a2, e2, two.n11.data(), two.edges.data());
        if (two.cnt != n || two.n11 != whole.n11 || two.edges != whole.edges) return fail("merge is not associative", L, n);
      }
      std::vector<uint64_t> left1(whole.n11.size(), 0u), right1(whole.n11.size(), 0u);
      epv::corr_part_close(R, L, samples, n, got.n11.data(), got.edges.data(), left1.data(), right1.data());
      for (uint32_t r = 0; r < R; ++r)
        for (uint32_t d = 0; d <= L; ++d) {
          uint64_t l = 0, rr = 0;
          for (const auto &sample : xs)
            for (uint64_t i = 0; i + d < n; ++i) { l += sample[r][i]; rr += sample[r][i + d]; }
          const size_t at = (size_t)r * (L + 1u) + d;
          if (left1[at] != l || right1[at] != rr) return fail("close differs from the count", L, n);
          if (got.n11[at] > l || got.n11[at] > rr || l + rr - got.n11[at] > samples * (n - d)) return fail("a bound fails", L, n);
        }
      // a piece shorter than max_lag is refused
      if (L > 1u) {
        std::vector<uint64_t> shortc(cnts);
        shortc[0] = L - 1u;
        bool threw = false;
        try {
          epv::corr_parts_merge(k, R, L, samples, shortc.data(), ap.data(), ep.data(), got.n11.data(), got.edges.data());
        } catch (const std::exception &) { threw = true; }
        if (!threw) return fail("a short piece was taken", L, n);
      }
    }
  std::puts("ok");
  return 0;
}
