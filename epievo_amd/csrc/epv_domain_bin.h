// epv_domain_bin.h -- the run-length bins of the domain size spectra, one definition for the device code
// (epv_domains.h) and the host code (host/epv_domains.cpp).  bin(l) = l for l < 16 (bin 0 is never used);
// otherwise, with e = floor(log2 l), bin(l) = 16 + 4 (e - 4) + ((l >> (e - 2)) & 3): exact up to 15, then four
// bins per octave.  Site indices fit 32 bits, so l < 2^32 and the last bin is 127.
#ifndef EPV_DOMAIN_BIN_H
#define EPV_DOMAIN_BIN_H

#include <stdint.h>

#define EPV_DOM_BINS 128u
// an edge record (the two runs a stretch of sites cannot close): bits 0-61 the length, bit 62 "whole" (the
// stretch holds no end at all; both records are then equal and the length is the stretch's), bit 63 the state
#define EPV_DOM_STATE_SHIFT 63
#define EPV_DOM_WHOLE (1ull << 62)
#define EPV_DOM_LEN_MASK ((1ull << 62) - 1ull)
#define EPV_DOM_MAX_SAMPLES (1ull << 21)

#if defined(__HIPCC__)
#define EPV_DOM_HD __host__ __device__
#else
#define EPV_DOM_HD
#endif

EPV_DOM_HD static inline uint32_t epv_domain_bin(uint64_t l) {
  if (l < 16u) return (uint32_t)l;
  const uint32_t e = 63u - (uint32_t)__builtin_clzll(l);
  const uint32_t b = 16u + 4u * (e - 4u) + (uint32_t)((l >> (e - 2u)) & 3u);
  return b < EPV_DOM_BINS ? b : EPV_DOM_BINS - 1u;   // (l >= 2^32 never arises from 32-bit site indices)
}

#endif
