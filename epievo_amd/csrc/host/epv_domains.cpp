// epv_domains.cpp -- see epv_domains.hpp
#include "epv_domains.hpp"

#include <algorithm>

namespace epv {

void domain_bin_range(uint32_t b, uint64_t *lo, uint64_t *hi) {
  if (b < 16u || b >= EPV_DOM_BINS) {
    *lo = *hi = b < 16u ? b : 0u;
    return;
  }
  const uint32_t e = 4u + (b - 16u) / 4u, q = (b - 16u) % 4u;
  *lo = (uint64_t)(4u + q) << (e - 2u);
  *hi = *lo + (1ull << (e - 2u)) - 1u;
}

namespace {
inline void bin_run(uint64_t *hist, uint64_t *len_sum, uint32_t v, uint64_t state, uint64_t len) {
  hist[((uint64_t)v * 2u + state) * EPV_DOM_BINS + epv_domain_bin(len)] += 1u;
  len_sum[(uint64_t)v * 2u + state] += len;
}
}  // namespace

void domain_parts_merge(uint64_t n_parts, uint32_t N, uint64_t samples, const uint64_t *const *hists,
                        const uint64_t *const *len_sums, const uint64_t *const *edges, uint64_t *out_hist,
                        uint64_t *out_len_sum, uint64_t *out_edges) {
  std::fill(out_hist, out_hist + (uint64_t)N * 2u * EPV_DOM_BINS, 0u);
  std::fill(out_len_sum, out_len_sum + (uint64_t)N * 2u, 0u);
  for (uint64_t p = 0; p < n_parts; ++p) {
    for (uint64_t i = 0; i < (uint64_t)N * 2u * EPV_DOM_BINS; ++i) out_hist[i] += hists[p][i];
    for (uint64_t i = 0; i < (uint64_t)N * 2u; ++i) out_len_sum[i] += len_sums[p][i];
  }
  for (uint64_t s = 0; s < samples; ++s)
    for (uint32_t v = 0; v < N; ++v) {
      const uint64_t at = (s * N + v) * 2u;
      bool open = false, closed = false;
      uint64_t open_state = 0, open_len = 0, first = 0;
      // a run is closed: the first one becomes the union's first record, the others are binned
      auto close = [&](uint64_t state, uint64_t len) {
        if (!closed) { first = len | (state << EPV_DOM_STATE_SHIFT); closed = true; }
        else bin_run(out_hist, out_len_sum, v, state, len);
      };
      for (uint64_t p = 0; p < n_parts; ++p) {
        const uint64_t f = edges[p][at], l = edges[p][at + 1u];
        if (!f && !l) continue;   // a part of no sites
        const uint64_t fs = f >> EPV_DOM_STATE_SHIFT, fl = f & EPV_DOM_LEN_MASK;
        if (f & EPV_DOM_WHOLE) {
          if (open && open_state == fs) { open_len += fl; continue; }
          if (open) close(open_state, open_len);
          open = true; open_state = fs; open_len = fl;
          continue;
        }
        if (open && open_state == fs) close(fs, open_len + fl);
        else {
          if (open) close(open_state, open_len);
          close(fs, fl);
        }
        open = true; open_state = l >> EPV_DOM_STATE_SHIFT; open_len = l & EPV_DOM_LEN_MASK;
      }
      if (!open) { out_edges[at] = out_edges[at + 1u] = 0u; continue; }
      const uint64_t last = open_len | (open_state << EPV_DOM_STATE_SHIFT);
      out_edges[at] = closed ? first : last | EPV_DOM_WHOLE;
      out_edges[at + 1u] = closed ? last : last | EPV_DOM_WHOLE;
    }
}

void domain_part_close(uint32_t N, uint64_t samples, uint64_t *hist, uint64_t *len_sum, const uint64_t *edges) {
  for (uint64_t s = 0; s < samples; ++s)
    for (uint32_t v = 0; v < N; ++v) {
      const uint64_t f = edges[(s * N + v) * 2u], l = edges[(s * N + v) * 2u + 1u];
      if (!f && !l) continue;
      bin_run(hist, len_sum, v, f >> EPV_DOM_STATE_SHIFT, f & EPV_DOM_LEN_MASK);
      if (!(f & EPV_DOM_WHOLE)) bin_run(hist, len_sum, v, l >> EPV_DOM_STATE_SHIFT, l & EPV_DOM_LEN_MASK);
    }
}

}  // namespace epv
