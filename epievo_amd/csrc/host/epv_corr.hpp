// epv_corr.hpp -- spatial correlations on the host: how the PARTS that contexts, shards and GPUs count
// (include/epievo_mi355x.h, epv_set_spatial_correlation) become the result.  Pure functions, no GPU.
//   R = N + B rows, L = max_lag (1 .. 1024), LW = ceil(L / 64)
//   a part over cnt >= L sites: n11 [R][L + 1], edges [samples][R][2][LW] (uint64): record 0 the first L bits of the
//   row (bit j = X[j]), record 1 the last L (bit j = X[cnt - L + j]); the spare bits of the last word are zero
// Identities (tests/test_spatial_correlation.py): merge(parts of the pieces) = part(concatenation); merging is
// associative; after close n11 <= min(left1, right1), left1 + right1 - n11 <= pairs, and at d = 0 all three are the
// ones of the row.
#ifndef EPV_CORR_HPP
#define EPV_CORR_HPP

#include <cstdint>

namespace epv {

constexpr uint32_t kCorrMaxLag = 1024;

inline uint32_t corr_edge_words(uint32_t L) { return (L + 63u) / 64u; }

// parts in genome order, each of cnts[p] >= L sites (a shorter one throws: a pair would span three parts).  The
// pairs that cross a boundary are counted from the left part's tail and the right part's head; the head of the
// union is the first part's, the tail the last part's.  out_* may not alias the inputs; returns the union's sites
uint64_t corr_parts_merge(uint64_t n_parts, uint32_t R, uint32_t L, uint64_t samples, const uint64_t *cnts,
                          const uint64_t *const *n11s, const uint64_t *const *edges, uint64_t *out_n11,
                          uint64_t *out_edges);

// a part over the whole genome of n sites -> left1, right1 [R][L + 1]: the ones at the left and at the right site of
// the pairs of every lag (n11 and edges are only read).  pairs[d] = samples (n - d)
void corr_part_close(uint32_t R, uint32_t L, uint64_t samples, uint64_t n, const uint64_t *n11, const uint64_t *edges,
                     uint64_t *left1, uint64_t *right1);

}  // namespace epv

#endif
