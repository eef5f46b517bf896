// epv_turnover_rec.h -- the edge record of the domain turnover, one definition for the device code
// (epv_turnover.h) and the host code (host/epv_turnover.cpp).  The record of the domain size spectra
// (epv_domain_bin.h) with one more flag: bits 0-60 the length, bit 61 "kept" (a site of the run has no net change
// on the branch), bit 62 "whole", bit 63 the state.  The bins are epv_domain_bin's.
#ifndef EPV_TURNOVER_REC_H
#define EPV_TURNOVER_REC_H

#include "epv_domain_bin.h"

#define EPV_TURN_KEPT_SHIFT 61
#define EPV_TURN_KEPT (1ull << EPV_TURN_KEPT_SHIFT)
#define EPV_TURN_LEN_MASK (EPV_TURN_KEPT - 1ull)
#define EPV_TURN_MAX_SAMPLES (1ull << 21)

#endif
