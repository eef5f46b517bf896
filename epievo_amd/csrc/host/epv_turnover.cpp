// epv_turnover.cpp -- see epv_turnover.hpp
#include "epv_turnover.hpp"

#include <algorithm>

namespace epv {

namespace {
struct Run {
  uint64_t state = 0, kept = 0, len = 0;
};
inline Run unpack(uint64_t rec) {
  Run r;
  r.state = rec >> EPV_DOM_STATE_SHIFT;
  r.kept = (rec >> EPV_TURN_KEPT_SHIFT) & 1u;
  r.len = rec & EPV_TURN_LEN_MASK;
  return r;
}
inline uint64_t pack(const Run &r) {
  return r.len | (r.kept << EPV_TURN_KEPT_SHIFT) | (r.state << EPV_DOM_STATE_SHIFT);
}
inline void bin_run(uint64_t *hist, uint64_t *len_sum, uint32_t r, const Run &x) {
  const uint64_t cls = ((uint64_t)r * 2u + x.state) * 2u + x.kept;
  hist[cls * EPV_DOM_BINS + epv_domain_bin(x.len)] += 1u;
  len_sum[cls] += x.len;
}
}  // namespace

void turnover_parts_merge(uint64_t n_parts, uint32_t R, uint64_t samples, const uint64_t *const *hists,
                          const uint64_t *const *len_sums, const uint64_t *const *edges, uint64_t *out_hist,
                          uint64_t *out_len_sum, uint64_t *out_edges) {
  const uint64_t nh = (uint64_t)R * 4u * EPV_DOM_BINS, nl = (uint64_t)R * 4u;
  std::fill(out_hist, out_hist + nh, 0u);
  std::fill(out_len_sum, out_len_sum + nl, 0u);
  for (uint64_t p = 0; p < n_parts; ++p) {
    for (uint64_t i = 0; i < nh; ++i) out_hist[i] += hists[p][i];
    for (uint64_t i = 0; i < nl; ++i) out_len_sum[i] += len_sums[p][i];
  }
  for (uint64_t s = 0; s < samples; ++s)
    for (uint32_t r = 0; r < R; ++r) {
      const uint64_t at = (s * R + r) * 2u;
      bool open = false, closed = false;
      Run cur;
      uint64_t first = 0;
      // a run is closed: the first one becomes the union's first record, the others are binned
      auto close = [&](const Run &x) {
        if (!closed) { first = pack(x); closed = true; }
        else bin_run(out_hist, out_len_sum, r, x);
      };
      for (uint64_t p = 0; p < n_parts; ++p) {
        const uint64_t f = edges[p][at], l = edges[p][at + 1u];
        if (!f && !l) continue;   // a part of no sites
        const Run fr = unpack(f);
        if (f & EPV_DOM_WHOLE) {
          if (open && cur.state == fr.state) { cur.len += fr.len; cur.kept |= fr.kept; continue; }
          if (open) close(cur);
          open = true; cur = fr;
          continue;
        }
        if (open && cur.state == fr.state) {
          cur.len += fr.len; cur.kept |= fr.kept;
          close(cur);
        } else {
          if (open) close(cur);
          close(fr);
        }
        open = true; cur = unpack(l);
      }
      if (!open) { out_edges[at] = out_edges[at + 1u] = 0u; continue; }
      const uint64_t last = pack(cur);
      out_edges[at] = closed ? first : last | EPV_DOM_WHOLE;
      out_edges[at + 1u] = closed ? last : last | EPV_DOM_WHOLE;
    }
}

void turnover_part_close(uint32_t R, uint64_t samples, uint64_t *hist, uint64_t *len_sum, const uint64_t *edges) {
  for (uint64_t s = 0; s < samples; ++s)
    for (uint32_t r = 0; r < R; ++r) {
      const uint64_t f = edges[(s * R + r) * 2u], l = edges[(s * R + r) * 2u + 1u];
      if (!f && !l) continue;
      bin_run(hist, len_sum, r, unpack(f));
      if (!(f & EPV_DOM_WHOLE)) bin_run(hist, len_sum, r, unpack(l));
    }
}

}  // namespace epv
