// epv_tracts.hpp -- change tracts on the host: how the PARTS that contexts, shards and GPUs count
// (include/epievo_mi355x.h, epv_set_change_tracts) become the result, and the file of epievo_est_histories -X.
// Pure functions, no GPU.
//   hist [B][27][128], len_sum [B][27], edges [samples][B][2] (uint64; classes and the record's bits:
//   epv_tract_rec.h)
// merge: tracts joined across a cut add their lengths and OR their direction bits, take the left flank of the
// leftmost piece and the right flank of the rightmost; a tract that ends at a cut takes the neighbour's boundary
// state as its flank.  close: the tracts still open at the two ends are binned with flank 2 (none).
// Identities (tests/test_change_tracts.py): merge(parts of the pieces) = part(concatenation), records included;
// merging is associative; after close, len_sum over the classes adds up to the changed sites of every branch.
#ifndef EPV_TRACTS_HPP
#define EPV_TRACTS_HPP

#include <cstdint>
#include <string>
#include <vector>

#include "../epv_tract_rec.h"

namespace epv {

// out_* may not alias the inputs; out_edges [samples][B][2]
void tract_parts_merge(uint64_t n_parts, uint32_t B, uint64_t samples, const uint64_t *const *hists,
                       const uint64_t *const *len_sums, const uint64_t *const *edges, uint64_t *out_hist,
                       uint64_t *out_len_sum, uint64_t *out_edges);

// in place: hist and len_sum become the result (edges are only read)
void tract_part_close(uint32_t B, uint64_t samples, uint64_t *hist, uint64_t *len_sum, const uint64_t *edges);

// the change tracts of epievo_est_histories -X (the closed result), integers only:
//   "#samples\t<S>\tbins\t128", then per branch "BRANCH:<child node name>", per class with a nonzero count a line
//   "<gain|loss|mixed>\tleft\t<0|1|->\tright\t<0|1|->\ttracts\t<count>\tsites\t<len_sum>" and one line
//   "lo\thi\tcount" per nonzero bin.  hist: [b][class][bin], len_sum: [b][class] (uint64)
struct ChangeTracts {
  uint64_t n_samples = 0;
  std::vector<std::string> branch_names;
  std::vector<uint64_t> hist;      // [B][27][128]
  std::vector<uint64_t> len_sum;   // [B][27]
};
void write_change_tracts(const std::string &file, const std::vector<std::string> &branch_names, uint64_t n_samples,
                         const uint64_t *hist, const uint64_t *len_sum);
ChangeTracts read_change_tracts(const std::string &file);

}  // namespace epv

#endif
