// epv_tract_rec.h -- the classes and the edge record of the change tracts, one definition for the device code
// (epv_tracts.h) and the host code (host/epv_tracts.cpp).  The bins are epv_domain_bin's.
//
// A tract is a maximal run of sites with a net change on a branch.  Its class is direction * 9 + left * 3 + right:
// direction 0 = gain (every end state 1), 1 = loss (every end state 0), 2 = mixed; a flank is the state of the
// unchanged site next to the tract, 2 where the tract touches the genome's first or last counted site.
//
// A stretch of sites has two records, [0] for its first site and [1] for its last:
//   bits 0-55  the length of the tract that holds the boundary site (0: the site is unchanged)
//   bit 56     the end state y of the boundary site (what a neighbouring stretch takes as its flank when the length is 0)
//   bit 57     the tract has a gained site        bit 58  the tract has a lost site
//   bit 59     the state of the unchanged site that bounds the tract inside the stretch (0 when whole or length 0)
//   bit 62     "whole": every site of the stretch changed; both records carry the stretch's length and direction bits
//   bit 63     set in both records of a stretch of at least one site: an empty stretch has both records 0
#ifndef EPV_TRACT_REC_H
#define EPV_TRACT_REC_H

#include "epv_domain_bin.h"

#define EPV_TRACT_DIRS 3u
#define EPV_TRACT_CLASSES 27u
#define EPV_TRACT_NONE 2u   /* the flank of a tract at a genome end */
#define EPV_TRACT_LEN_MASK ((1ull << 56) - 1ull)
#define EPV_TRACT_Y_SHIFT 56
#define EPV_TRACT_GAIN_SHIFT 57
#define EPV_TRACT_LOSS_SHIFT 58
#define EPV_TRACT_FLANK_SHIFT 59
#define EPV_TRACT_WHOLE (1ull << 62)
#define EPV_TRACT_SET (1ull << 63)
#define EPV_TRACT_MAX_SAMPLES (1ull << 21)

// gain only -> 0, loss only -> 1, both -> 2
EPV_DOM_HD static inline uint32_t epv_tract_dir(uint32_t gain, uint32_t loss) { return loss ? (gain ? 2u : 1u) : 0u; }
EPV_DOM_HD static inline uint32_t epv_tract_class(uint32_t dir, uint32_t left, uint32_t right) {
  return dir * 9u + left * 3u + right;
}

#endif
