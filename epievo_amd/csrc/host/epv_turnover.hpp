// epv_turnover.hpp -- domain turnover on the host: how the PARTS that contexts, shards and GPUs count
// (include/epievo_mi355x.h, epv_set_domain_turnover) become the result.  Pure functions, no GPU.
//   R = 2 B rows: row 2 b the start of branch b (the parent's state as the branch sees it), row 2 b + 1 its end
//   hist [R][2 state][2 kept][128], len_sum [R][2][2], edges [samples][R][2] (uint64; the record's bits:
//   epv_turnover_rec.h)
// merge and close are those of the domain size spectra (epv_domains.hpp) with one addition: a run joined from
// pieces is kept iff any piece is kept.
// Identities (tests/test_domain_turnover.py): merge(parts of the pieces) = part(concatenation); merging is
// associative; after close, len_sum over state and kept adds up to the sites of every row.
#ifndef EPV_TURNOVER_HPP
#define EPV_TURNOVER_HPP

#include <cstdint>

#include "../epv_turnover_rec.h"

namespace epv {

// out_* may not alias the inputs; out_edges [samples][R][2]
void turnover_parts_merge(uint64_t n_parts, uint32_t R, uint64_t samples, const uint64_t *const *hists,
                          const uint64_t *const *len_sums, const uint64_t *const *edges, uint64_t *out_hist,
                          uint64_t *out_len_sum, uint64_t *out_edges);

// in place: hist and len_sum become the result (edges are only read)
void turnover_part_close(uint32_t R, uint64_t samples, uint64_t *hist, uint64_t *len_sum, const uint64_t *edges);

}  // namespace epv

#endif
