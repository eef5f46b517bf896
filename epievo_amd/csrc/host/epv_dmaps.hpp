// epv_dmaps.hpp -- domain maps on the host: the membership rule itself, the PART a stretch of sites contributes
// (include/epievo_mi355x.h, epv_set_domain_maps), how adjacent parts merge, and the file of epievo_est_histories -D.
// Pure functions, no GPU.
//   N nodes, K sizes L_1 < .. < L_K (1 .. 1024, K <= 4), E = 2 (L_K - 1) bits of an edge record, EW = ceil(E / 64)
//   a part over cnt >= E sites: counts [N][K][cnt] (uint32), edges [samples][N][2][EW] (uint64): record 0 the first E
//   bits of the row (bit j = row[j]), record 1 the last E (bit j = row[cnt - E + j]); spare bits zero
// A row is the indicator of "the node is in the state asked for": the functions here never see the state.
// Identities (tests/test_domain_maps.py): merge(parts of the pieces) = part(concatenation), for counts and records
// alike; merging is associative.
#ifndef EPV_DMAPS_HPP
#define EPV_DMAPS_HPP

#include <cstdint>
#include <string>
#include <vector>

namespace epv {

constexpr uint32_t kDmapsMaxSize = 1024, kDmapsMaxSizes = 4;

inline uint32_t dmaps_edge_bits(uint32_t LK) { return 2u * (LK - 1u); }
inline uint32_t dmaps_edge_words(uint32_t LK) { return (dmaps_edge_bits(LK) + 63u) / 64u; }

// 1 .. 4 strictly increasing sizes of 1 .. 1024, or it throws (`who` opens the message)
void check_domain_map_sizes(uint32_t K, const uint32_t *sizes, const char *who);

// the opening of the bit string x (nbits bits in ceil(nbits / 64) words, spare bits zero) by L >= 1: out bit p = 1
// where p lies in a run of at least L ones.  Erode by L, dilate by L, spans doubling.  out may not alias x
void domain_map_members(const uint64_t *x, uint64_t nbits, uint32_t L, uint64_t *out);

// one sample over a stretch of cnt sites: bits [N][ceil(cnt / 64)] the rows (spare bits zero); counts [N][K][cnt]
// receives + 1 per membership, edges [N][2][EW] this sample's records.  The CPU twin of epv_dmaps_member_kernel
void domain_maps_part(uint32_t N, uint32_t K, const uint32_t *sizes, uint64_t cnt, const uint64_t *bits,
                      uint32_t *counts, uint64_t *edges);

// parts in genome order, each of cnts[p] >= E sites (a shorter one throws).  out_counts [N][K][sum of cnts],
// out_edges [samples][N][2][EW]; neither may alias an input.  Returns the union's sites
uint64_t domain_maps_merge(uint64_t n_parts, uint32_t N, uint32_t K, const uint32_t *sizes, uint64_t samples,
                           const uint64_t *cnts, const uint32_t *const *counts, const uint64_t *const *edges,
                           uint32_t *out_counts, uint64_t *out_edges);

// sums [N][K][ceil(n / W)] of counts [N][K][n] over windows of W consecutive sites
void domain_map_windows(uint32_t N, uint32_t K, uint64_t n, const uint32_t *counts, uint64_t W, uint64_t *sums);

// the file of epievo_est_histories -D, integers only:
//   #samples <S> state <s> sizes <L_1> .. <L_K>
//   #window <W> sites <n>
//   then per node "NODE:<name>" and one line per window: its K sums
struct DomainMaps {
  uint64_t n_samples = 0, n_sites = 0, window = 0;
  uint32_t state = 0;
  std::vector<uint32_t> sizes;
  std::vector<std::string> node_names;
  std::vector<uint64_t> sums;   // [N][K][windows]
};
void write_domain_maps(const std::string &file, const std::vector<std::string> &node_names, uint64_t n_samples,
                       uint32_t state, const std::vector<uint32_t> &sizes, uint64_t n_sites, uint64_t W,
                       const uint64_t *sums);
DomainMaps read_domain_maps(const std::string &file);

}  // namespace epv

#endif
