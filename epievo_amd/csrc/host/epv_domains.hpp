// epv_domains.hpp -- domain size spectra on the host: the bins, and how the PARTS that contexts, shards and
// GPUs count (include/epievo_mi355x.h, epv_set_domain_stats) become the result.  Pure functions, no GPU.
//   hist [N][2][128], len_sum [N][2], edges [samples][N][2] (uint64; the edge record's bits: epv_domain_bin.h)
// merge: adjacent parts, in genome order, give the part of their union.  hist and len_sum are added; then, per
//   sample and node, the parts are walked with one open run.  A whole part extends an open run of its state (of
//   the other state: the open run is closed and the whole part becomes the open run).  Otherwise the part's
//   first record is joined to an open run of its state and closed (of the other state: both are closed
//   separately), and the part's last record becomes the open run.  The first run closed this way is not binned:
//   it becomes the union's first record.  Nothing ever closed: the union is whole.  Parts of no sites (both
//   records 0) are skipped.
// close: the first and last records are binned and added; a whole record once.
// Identities (tests/test_domain_stats.py): merge(parts of the pieces) = part(concatenation); merging is
// associative; after close, the two states' len_sum add up to the sites.
#ifndef EPV_DOMAINS_HPP
#define EPV_DOMAINS_HPP

#include <cstdint>

#include "../epv_domain_bin.h"

namespace epv {

// the inclusive range of run lengths of bin b (1 <= b <= 127); bin 0 holds nothing: lo = hi = 0
void domain_bin_range(uint32_t b, uint64_t *lo, uint64_t *hi);

// out_* may not alias the inputs; out_edges [samples][N][2]
void domain_parts_merge(uint64_t n_parts, uint32_t N, uint64_t samples, const uint64_t *const *hists,
                        const uint64_t *const *len_sums, const uint64_t *const *edges, uint64_t *out_hist,
                        uint64_t *out_len_sum, uint64_t *out_edges);

// in place: hist and len_sum become the result (edges are only read)
void domain_part_close(uint32_t N, uint64_t samples, uint64_t *hist, uint64_t *len_sum, const uint64_t *edges);

}  // namespace epv

#endif
