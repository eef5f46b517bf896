// epv_part.h -- the shape of a PART: what a context keeps of a summary that is joint along the genome (the domain
// size spectra, the domain turnover, the spatial correlations, the domain maps, the change tracts; DESIGN.md
// section 7.26).  One sample's bit rows (epv_rows.h) in a scratch, one or two accumulators over the samples, and per
// sample the edge records of what the context's stretch of sites cannot close.  Every byte size of a part is
// computed here, once, when the part is laid out; epv_abi.hip allocates, zeroes and copies by these sizes alone.
// Host code without HIP: tools/part_shape_check.cpp compiles it on the CPU.
#ifndef EPV_PART_H
#define EPV_PART_H

#include <stddef.h>
#include <stdint.h>

#include "epv_tract_rec.h"   // EPV_TRACT_CLASSES (and, through it, EPV_DOM_BINS)

struct PartShape {
  uint32_t rows = 0;          // bit rows of one sample
  uint64_t words = 0;         // 64-site words of a row
  size_t bits_b = 0;          // the scratch [rows][words]
  size_t edge_b = 0;          // one sample's edge records
  size_t edges_b = 0;         // ... of all the samples the part is allocated for
  size_t acc_b[2] = {0, 0};   // the accumulators over the samples (0: none)
  size_t total() const { return bits_b + edges_b + acc_b[0] + acc_b[1]; }
};

// rows over cnt sites, edge_b bytes of edge records per sample for max samples, two accumulators
inline PartShape part_shape(uint32_t rows, uint64_t cnt, uint64_t max, size_t edge_b, size_t acc0_b, size_t acc1_b) {
  PartShape p;
  p.rows = rows;
  p.words = (cnt + 63u) / 64u;
  p.bits_b = (size_t)8u * rows * p.words;
  p.edge_b = edge_b;
  p.edges_b = edge_b * max;
  p.acc_b[0] = acc0_b;
  p.acc_b[1] = acc1_b;
  return p;
}
// domain size spectra: hist [N][2][128], len [N][2]; edge [N][2]
inline PartShape domains_shape(uint32_t N, uint64_t cnt, uint64_t max) {
  return part_shape(N, cnt, max, (size_t)16u * N, (size_t)16u * EPV_DOM_BINS * N, (size_t)16u * N);
}
// domain turnover, R = 2 B rows: hist [R][2][2][128], len [R][2][2]; edge [R][2]
inline PartShape turnover_shape(uint32_t B, uint64_t cnt, uint64_t max) {
  const uint32_t R = 2u * B;
  return part_shape(R, cnt, max, (size_t)16u * R, (size_t)32u * EPV_DOM_BINS * R, (size_t)32u * R);
}
// change tracts, the turnover's 2 B rows: hist [B][27][128], len [B][27]; edge [B][2]
inline PartShape tracts_shape(uint32_t B, uint64_t cnt, uint64_t max) {
  return part_shape(2u * B, cnt, max, (size_t)16u * B, (size_t)8u * EPV_TRACT_CLASSES * EPV_DOM_BINS * B,
                    (size_t)8u * EPV_TRACT_CLASSES * B);
}
// spatial correlations of max_lag L, R = N + B rows: n11 [R][L + 1]; edge [R][2][LW], LW = ceil(L / 64)
inline PartShape corr_shape(uint32_t N, uint32_t B, uint32_t L, uint64_t cnt, uint64_t max) {
  const uint32_t R = N + B, LW = (L + 63u) / 64u;
  return part_shape(R, cnt, max, (size_t)16u * R * LW, (size_t)8u * R * (L + 1u), 0u);
}
// domain maps of K sizes, the largest LK: counts uint32 [N][K][cnt]; edge [N][2][EW], EW = ceil(2 (LK - 1) / 64)
inline uint32_t dmaps_edge_bits(uint32_t LK) { return 2u * (LK - 1u); }
inline PartShape dmaps_shape(uint32_t N, uint32_t K, uint32_t LK, uint64_t cnt, uint64_t max) {
  const uint32_t EW = (dmaps_edge_bits(LK) + 63u) / 64u;
  return part_shape(N, cnt, max, (size_t)16u * N * EW, (size_t)4u * N * K * cnt, 0u);
}

#endif
