// epv_epochs.hpp -- closing the epoch statistics' difference form (csrc/epv_epochs.h, epv_get_epoch_stats)
// on the host, in exact integers.  No GPU code.
#ifndef EPV_EPOCHS_HPP
#define EPV_EPOCHS_HPP

#include <cstdint>

namespace epv {

// out[p] = floor(p fixT / P) for p = 0 .. P-1 (E_P = +inf is not stored); fixT < 2^50, P >= 1
void epoch_edges(uint64_t fixT, uint32_t P, uint64_t *out);

// raw[B][P][32] uint64 (J[8], lo[8], hi[8], cov[8] two's complement; part = lo + 2^32 hi, words added
// modulo 2^64 over any number of contexts whose own words did not wrap) -> closed[B][P][24]:
// J[8] as int64, then D[8] as 128-bit integers, low words [8] then high words [8]:
//   D[p] = part[p] + (E_{p+1} - E_p) sum_{q <= p} cov[q]     (the last bin is never covered wholly)
// throws std::runtime_error where the difference form is not one a walk can have made (a negative cover count,
// cover in the last bin)
void epoch_close(const uint64_t *raw, const uint64_t *fixT, uint32_t B, uint32_t P, uint64_t *closed);

// closed[B][P][24] -> J, D[B][P][8] per sample, D in time units (k[b] = k_b of the non-root nodes)
void epoch_counts_to_stats(const uint64_t *closed, const int *k, uint32_t B, uint32_t P, uint64_t samples, double *J,
                           double *D);

}  // namespace epv

#endif
