#ifndef EPV_DIRECT_H
#define EPV_DIRECT_H
// epv_direct.h -- the direct end-conditioned sampler of a segment (included by epv_kernels.h; DESIGN.md
// section 7.22).  EPV_OPT_DIRECT_SAMPLER selects it: the jump times of a segment of the two-state chain given
// its start state, its end state and its rates, drawn from the conditional law itself instead of searched for
// among forward trials.  Work is O(jumps drawn) and every loop is counted, so a segment ALWAYS returns --
// forward rejection on a kept state, and Nielsen's method after its first jump, need about exp(rate T) trials
// where a state is left fast and re-entered slowly.
//
// With s the time left, a the state, b the target, ra the rate of leaving a, rb of the other state, l = ra + rb:
//   a == b  no further jump with probability p0 = exp(-ra s) / Paa(s), Paa(s) = (rb + ra exp(-l s)) / l;
//           otherwise the next jump tau has density ~ exp(-ra tau) (1 - exp(-l (s - tau))): proposed from the
//           truncated exponential (Nielsen's transform) and accepted when v (1 - exp(-l s)) < 1 - exp(-l (s - tau)).
//           The proposal density decreases and the acceptance is concave from 1 down to 0: a round succeeds
//           with probability >= 1/2 whatever the rates and the length.
//   a != b  the next jump has density ~ ra/l exp(-ra tau) + rb/l exp(-ra s) exp(-rb (s - tau)): a mixture of a
//           truncated exponential in tau (weight w1 = 1 - exp(-ra s)) and one in s - tau (weight
//           w2 = exp(-ra s) (1 - exp(-rb s))), drawn by inversion: one uniform picks the arm, one inverts.
// After a jump the chain stands in the other state at base + tau and the same step repeats.
//
// Random stream (the row "direct sampler" of epv_philox.h): draw 0 is trial 1's first draw, later draws fill
// blocks 0 .. 253 of trial words 1, 2, ...; the draws of a segment are consumed in order, whatever they decide.
//
// Bounds: the outer loop runs at most room + 1 times (a jump beyond `room` is TRIAL_OVERFLOW), a jump is
// drawn in at most EPV_DIRECT_ROUNDS rounds (a round whose time does not land strictly inside the segment counts
// as failed, which also covers NaN: every comparison is then false), after which the segment gives up
// (TRIAL_GIVEUP: the caller rejects the proposal and counts it, epv_direct_giveups).

#define TRIAL_GIVEUP 3
#define EPV_DIRECT_ROUNDS 64u     /* rounds per jump: a round fails with probability <= 1/2 */
#define EPV_DIRECT_WORD_DRAWS 508u /* draws per trial word: blocks 0 .. 253, two draws each */
#define EPV_DIRECT_MAX_ROOM 4096u  /* the outer loop's bound whatever the caller passes (capacity <= 2047) */

struct epv_direct_stream {
  uint32_t seed_lo, seed_hi, gsite, sweep, node, k, d;
  epv_block2 blk;
  __device__ __forceinline__ double next() {
    double u;
    if (d == 0u) {
      u = epv_keyed_block(seed_lo, seed_hi, gsite, sweep, node, k, 0u, 0u).d1;
    } else {
      const uint32_t e = d - 1u;
      if ((e & 1u) == 0u) {
        const uint32_t w = e / EPV_DIRECT_WORD_DRAWS;
        blk = epv_keyed_block(seed_lo, seed_hi, gsite, sweep, node, k, 1u + w, (e - w * EPV_DIRECT_WORD_DRAWS) >> 1);
      }
      u = (e & 1u) ? blk.d1 : blk.d0;
    }
    ++d;
    return u;
  }
};

// run_trial's arguments without the trial: outcome, the jump count, stored times (the first `max_store` at
// dst[0], dst[stride], ..., + start_time); draws_out = uniforms consumed, run_out = the longest run of rounds
__device__ __forceinline__ int run_direct(uint32_t seed_lo, uint32_t seed_hi, uint32_t gsite, uint32_t sweep,
                                          uint32_t node, uint32_t k, uint32_t a0, uint32_t end, double T, double r0,
                                          double r1, uint32_t room, double *dst, uint64_t stride, uint32_t max_store,
                                          double start_time, uint32_t &nj_out, uint32_t &draws_out, uint32_t &run_out,
                                          uint32_t first_draw_index = 0u) {
  // first_draw_index (epv_direct_kat alone; the kernels pass none): the segment's draws begin at this index of its
  // stream instead of 0 -- 0 or odd, so that the first draw opens a block --, which lets a known-answer item cross
  // from one trial word into the next within a few jumps; draws_out is then the index after the last draw
  epv_direct_stream R;
  R.seed_lo = seed_lo; R.seed_hi = seed_hi; R.gsite = gsite; R.sweep = sweep; R.node = node; R.k = k; R.d = first_draw_index;
  R.blk.d0 = 0.0; R.blk.d1 = 0.0;
  if (room > EPV_DIRECT_MAX_ROOM) room = EPV_DIRECT_MAX_ROOM;
  const double lam = r0 + r1;
  uint32_t a = a0, nj = 0u, longest = 0u;
  double base = 0.0;
  int outcome = TRIAL_GIVEUP;
  for (uint32_t it = 0u; it <= room; ++it) {
    const double s = T - base;
    const double ra = a ? r1 : r0, rb = a ? r0 : r1;
    const double ea = epv_exp(-ra * s);
    double tn = 0.0;
    bool landed = false;
    uint32_t run = 0u;
    if (a == end) {
      const double el = epv_exp(-lam * s);
      const double p0 = ea / ((rb + ra * el) / lam);
      const double u0 = R.next();
      if (1.0 - u0 < p0) { outcome = TRIAL_OK; break; }
      if (nj >= room) { outcome = TRIAL_OVERFLOW; break; }
      const double w = 1.0 - ea, wl = 1.0 - el;
      for (uint32_t r = 0u; r < EPV_DIRECT_ROUNDS && !landed; ++r) {
        const double u = R.next();
        const double v = R.next();
        ++run;
        const double tau = -epv_log(1.0 - u * w) / ra;
        tn = base + tau;
        if (tau < s && tn > base && tn < T) landed = v * wl < 1.0 - epv_exp(-lam * (s - tau));
      }
    } else {
      if (nj >= room) { outcome = TRIAL_OVERFLOW; break; }
      const double eb = epv_exp(-rb * s);
      const double w1 = 1.0 - ea, wb = 1.0 - eb;
      const double w2 = ea * wb;
      for (uint32_t r = 0u; r < EPV_DIRECT_ROUNDS && !landed; ++r) {
        const double u = R.next();
        const double v = R.next();
        ++run;
        double tau;
        if (u * (w1 + w2) < w1) tau = -epv_log(1.0 - v * w1) / ra;
        else tau = s - -epv_log(1.0 - v * wb) / rb;
        tn = base + tau;
        landed = tau < s && tn > base && tn < T;
      }
    }
    longest = run > longest ? run : longest;
    if (!landed) break;     // TRIAL_GIVEUP
    a ^= 1u;
    if (nj < max_store) dst[(uint64_t)nj * stride] = tn + start_time;
    ++nj;
    base = tn;
  }
  nj_out = nj;
  draws_out = R.d;
  run_out = longest;
  return outcome;
}

#endif
