/* epievo_mi355x.h -- C ABI of the MI355X (gfx950) implementation of epievo's MCEM
 * inner loop: the per-site Metropolis-Hastings end-conditioned path sampler.
 *
 * The reference has no FFI; its boundary for this path is the C++ class
 * SingleSiteSampler (/root/reference/src/libepievo/SingleSiteSampler.hpp:35-81) plus
 * two free functions of ParamEstimation.hpp.  Each entry point below names the
 * reference interface it replaces.  The C++ wrapper epv::SingleSiteSampler
 * (epievo_amd/csrc/host/epv_sampler.hpp) keeps the reference's names and argument
 * meaning on top of this ABI; INTEGRATION.md shows the binding a maintainer adds.
 *
 * Conventions
 *  - plain pointers and sizes only; all buffers are caller-owned HOST memory unless a
 *    name ends in _dev (then it is a device pointer on the context's GPU);
 *  - every call returns 0 on success or a non-zero EPV_ERR_* code; the message is
 *    available from epv_last_error(ctx).  No exception crosses the boundary;
 *  - one context per GPU, calls on one context are serialised by the caller (the
 *    reference class is single-threaded and not re-entrant either);
 *  - paths are passed "node-major flat": for node b = 1..n_nodes-1 and site s the
 *    entry index is e = (b-1)*n_sites + s; init_state[e] is Path::init_state, the
 *    jumps are jumps[offsets[e] .. offsets[e+1]) (Path::jumps, ascending, absolute
 *    times in (0, branch length)).  Node 0 (the root) has no path, as in the
 *    reference where paths[site][0] is a dummy (epievo_est_params_histories.cpp:186-192);
 *  - J and D are per-branch sufficient statistics laid out [(b-1)*8 + ctx] with
 *    ctx = 4*left + 2*mid + right (epievo_utils.hpp:85-88).
 */
#ifndef EPIEVO_MI355X_H
#define EPIEVO_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct epv_ctx epv_ctx;

enum {
  EPV_OK = 0,
  EPV_ERR_ARG = 1,      /* bad argument / call order */
  EPV_ERR_HIP = 2,      /* a HIP runtime call failed (no device, OOM, ...) */
  EPV_ERR_CAPACITY = 3, /* a proposed path needed more than `capacity` jumps */
  EPV_ERR_STATE = 4     /* paths/model/tree not set */
};

/* counters returned by epv_get_counters */
typedef struct {
  uint64_t n_overflow;   /* proposals rejected because a branch exceeded `capacity` jumps */
  uint64_t n_coop_tasks; /* rejection tasks resolved by the wave-cooperative search */
  uint64_t n_sweeps;     /* colour-complete sweeps executed since create */
  uint64_t n_search_finished; /* of n_coop_tasks (fused phase): branches the segment search finished itself */
} epv_counters;

/* Run-time options of a context (epv_set_options; default 0).
 * EPV_OPT_REFERENCE_PROPOSAL_RATIO  evaluate the proposal ratio q(old)/q(new) of
 *     Metropolis_Hastings_site with the reference's sums (downward_sampling_branch,
 *     SingleSiteSampler.cpp:180-225, and proposal_prob_branch, :272-314).  With SAMPLE_ROOT false
 *     (hard-wired, :441) that ratio is EXACTLY 1: per segment the reference accumulates
 *     log(p[k+1][end] / p[k][start]), which telescopes along every branch and over the tree to the
 *     log of the proposal's normalising constant -- independent of the path.  The reference's
 *     value differs from 0 by rounding only; by default the kernels use the exact 0 and skip
 *     the sums (same paths, same statistics; tests/test_proposal_ratio.py).
 * EPV_OPT_FORWARD_REJECTION  sample state-changing segments by forward rejection
 *     (end_cond_sample_forward_rejection, EndCondSampling.cpp:479-509, the sampler the
 *     reference's hot path calls) instead of the reference library's
 *     end_cond_sampling_Nielsen (:576-617), the default here because its acceptance probability
 *     does not vanish on short branches.  Same conditional law; for parity tests.
 * EPV_OPT_SAMPLE_ROOT  the reference class's public field SAMPLE_ROOT (SingleSiteSampler.hpp:78): the
 *     proposal also draws the site's root state from its posterior given the neighbours' root
 *     states and the data below (root_post_prob0 / downward_sampling, SingleSiteSampler.cpp:167-176,
 *     :246-249) and both proposal log-probabilities carry the term (:325-329).  The reference
 *     hard-wires it to false (:441) and none of its programs sets it.  With it the proposal ratio
 *     is no longer identically 1, so the kernels evaluate it as under
 *     EPV_OPT_REFERENCE_PROPOSAL_RATIO (the first-generation proposal kernel; about half the
 *     default throughput).  Pinned: oracle rung A with the field set == the linked reference bit
 *     for bit; the GPU == rung B bit for bit (tests/test_sample_root.py).
 * EPV_OPT_DIRECT_SAMPLER  draw every segment's jump times from the conditional law itself (DESIGN.md section
 *     7.22, csrc/epv_direct.h) instead of searching forward trials for one that ends in the right state: a
 *     kept state stops with probability exp(-ra s) / Paa(s) or draws its next jump by a rejection that succeeds
 *     with probability >= 1/2 per round, a state change draws it by inversion from a two-arm mixture.  Work is
 *     O(jumps drawn) and every loop is counted, so a colour phase returns whatever the rates -- the default
 *     search needs about exp(rate T) trials where a state is left fast and re-entered slowly.  Same conditional
 *     law, another use of the random stream (not bit-comparable with the other two samplers; the CPU oracle has
 *     no such mode, tests/direct_ref.py restates it).  A colour phase then runs the separate jump-time kernels
 *     in their direct variants (plan bit 23; the fused phase only with EPV_OPT_DIRECT_FUSED).  A segment that exhausts its 64 rounds
 *     gives up: the proposal is rejected through the overflow flag and counted (epv_direct_giveups).  Together
 *     with EPV_OPT_FORWARD_REJECTION: EPV_ERR_ARG.  The initial paths of epv_init_paths_indep and
 *     the site-independent updates keep the default sampler.
 * EPV_OPT_DIRECT_FUSED  only together with EPV_OPT_DIRECT_SAMPLER (alone: EPV_ERR_ARG).  Wherever the default
 *     mode would run the fused phase, the direct mode runs it too, in the kernel's direct bodies: the wave samples
 *     its segment list by the same run_direct and assembles its branches itself, with no unbounded loop.  Same
 *     paths, statistics and counters as without the bit, bit for bit; where the fused phase is not eligible
 *     (a reference ratio, a sampled root, the large-tree kernel, a global pool, launches above the fused limit)
 *     the plan is that of EPV_OPT_DIRECT_SAMPLER alone.  So it is while a leaf cell is unobserved or carries
 *     evidence: the first kernel then, or under EPV_OPT_LEAF_FAST the leaf variant of the second or third, and
 *     the separate direct jump kernels either way (the fused direct bodies have no leaf variant).
 * EPV_OPT_LEAF_FAST  off by default.  A held leaf cell (epv_set_unobserved, epv_set_leaf_evidence) no longer
 *     sends the colour phases to the first proposal kernel: the plan is what the same context would get with no
 *     cell held -- the fused phase (generic or small-tree body, same sites per wave), the second kernel with its
 *     jump stage, or the third with its words and slab pool -- and plan bits 17 / 18, which stay set, select
 *     that kernel's leaf variant: the same kernel with the leaf vector (evidence, else the mask, else the
 *     indicator; the first kernel's precedence and device layouts) wherever it would take a leaf's observed
 *     state.  The first kernel stays wherever it is chosen for another reason: a
 *     reference ratio, EPV_OPT_SAMPLE_ROOT, EPV_PROPOSE_V1, a global pool without the third kernel, a tree the
 *     third does not take.  Same chain: the GPU equals oracle rung B bit for bit with the bit on as with it off
 *     (tests/test_leaf_fast_gpu.py).  With no cell held the plan word and every result are those of the bit
 *     off.  Combines freely with EPV_OPT_FORWARD_REJECTION and EPV_OPT_DIRECT_SAMPLER. */
enum { EPV_OPT_REFERENCE_PROPOSAL_RATIO = 1, EPV_OPT_FORWARD_REJECTION = 2, EPV_OPT_SAMPLE_ROOT = 4,
       EPV_OPT_DIRECT_SAMPLER = 8, EPV_OPT_DIRECT_FUSED = 16, EPV_OPT_LEAF_FAST = 32 };

/* Create a context on HIP device `device_id`.  Returns NULL when the device cannot be
 * initialised (the product has no CPU fallback).  Replaces
 * SingleSiteSampler::SingleSiteSampler (SingleSiteSampler.cpp:439-447). */
epv_ctx *epv_create(int device_id);
void epv_destroy(epv_ctx *ctx);
const char *epv_last_error(const epv_ctx *ctx);

/* Tree in pre-order array form = the fields of TreeHelper (TreeHelper.hpp:47-51):
 * subtree_sizes, parent_ids, branches (branches[0] = 0, the root). */
int epv_set_tree(epv_ctx *ctx, int n_nodes, const uint32_t *parent_ids,
                 const uint32_t *subtree_sizes, const double *branches);

/* Model = the two members of EpiEvoModel the sampler reads (EpiEvoModel.hpp:37-41):
 * triplet_rates[8] and the horizontal transition matrix T (row-major 2x2).
 * log(rate) is taken here on the host with libm, as reset() does
 * (SingleSiteSampler.cpp:464-468).  The call is ordered on the context's stream and does not wait for
 * the device: work queued before it reads the old constants, work queued after it the new ones. */
int epv_set_model(epv_ctx *ctx, const double *triplet_rates, const double *T);

/* Upload all paths (replaces handing `vector<vector<Path>>&` to reset()).
 * `capacity` is the fixed number of jump slots kept per (site, branch) on the device
 * (1..2047: a branch has at most 2 * capacity + 1 segments and the segment field of the random
 * stream's address has 12 bits); 0 picks max(16, 2*max_jumps_in_input + 8).  A proposal that would need
 * more is rejected and counted (epv_counters.n_overflow) and the MCMC call that saw it
 * returns EPV_ERR_CAPACITY after completing -- re-upload with a larger capacity.
 * `global_site_offset`: index of local site 0 in the whole genome (0 on one GPU);
 * it keys the RNG and the 3-colouring so that sharded runs reproduce unsharded ones. */
int epv_upload_paths(epv_ctx *ctx, uint64_t n_sites, const uint8_t *init_state,
                     const uint64_t *offsets, const double *jumps, uint32_t capacity,
                     uint64_t global_site_offset);

/* Change the number of jump slots per (site, branch) of the RESIDENT paths, on the device
 * (no host round trip): the jump planes are re-strided, states and cached log-likelihoods
 * stay valid.  The reference's std::vector paths grow on demand; this is the equivalent a
 * wrapper calls after EPV_ERR_CAPACITY (the run that reported it is a valid chain on the
 * histories with at most `capacity` jumps per branch).  Fails with EPV_ERR_CAPACITY when a
 * resident path has more jumps than `capacity`; capacity is clamped to 1..2047. */
int epv_set_capacity(epv_ctx *ctx, uint32_t capacity);
int epv_get_capacity(epv_ctx *ctx, uint32_t *capacity);
int epv_set_options(epv_ctx *ctx, uint32_t flags);
int epv_get_options(epv_ctx *ctx, uint32_t *flags);
/* Which kernels a colour phase of the resident paths launches (chosen by tree size, mean jumps per
 * branch and launch size; results are bit-identical in every mode) -- for profiles and bench lines:
 * 0 = epv_mh_propose_kernel + epv_mh_jumps_kernel + epv_mh_accept_kernel (reference
 *     proposal arithmetic), 1 = epv_mh_propose2_kernel + jumps + accept, 2 = epv_mh_propose2_kernel +
 *     epv_seg_search_kernel + epv_seg_assemble_kernel + accept (long branches), 3 = the fused phase:
 *     one epv_mh_propose2_kernel launch that also samples the jump times and accepts (launches of few
 *     waves), 4 = epv_mh_propose3_kernel + epv_mh_jumps_all_kernel + epv_mh_accept3_kernel (large trees:
 *     the tree walked level by level, heavy branches one lane each, a lane per (site, triple) in the
 *     acceptance).  No reference counterpart. */
enum { EPV_PHASE_V1 = 0, EPV_PHASE_V2 = 1, EPV_PHASE_V2_SEGMENTS = 2, EPV_PHASE_FUSED = 3, EPV_PHASE_V3 = 4 };
/* (Under EPV_OPT_DIRECT_SAMPLER the mode names the proposal kernel's family as above, but the jump stage runs its
 * direct variants: mode 1 launches epv_mh_jumps_direct_kernel, not epv_mh_jumps_all_kernel, mode 2 the direct search
 * and assembly kernels, and mode 3 is reported only with EPV_OPT_DIRECT_FUSED: the fused kernel's direct bodies.
 * epv_phase_plan's bit 23 tells the two apart.) */
int epv_phase_mode(epv_ctx *ctx, uint32_t *mode);

/* The exact kernel variants a colour phase of the resident paths launches, as one word (the launch
 * code reads the same plan; for tests and profiles).  Fields that do not apply to the chosen
 * proposal kernel are 0.
 *   bits 0-1   proposal kernel: EPV_PLAN_V1 (epv_mh_propose_kernel), EPV_PLAN_V2 (epv_mh_propose2_kernel),
 *              EPV_PLAN_V3 (epv_mh_propose3_kernel), EPV_PLAN_FUSED (epv_mh_propose2_kernel, fused phase)
 *   bit  2     V1: the record pool in global memory (0 = LDS)
 *   bit  3     V1: the reference proposal-ratio template (EPV_OPT_REFERENCE_PROPOSAL_RATIO, EPV_OPT_SAMPLE_ROOT)
 *   bits 4-7   fused: the small-tree body's node count NN (2 .. 5), 0 = the generic body
 *   bits 8-9   V3: 64-bit words per node mask (1 for trees of at most 64 nodes, else 2)
 *   bit  10    V3: slabs from the per-XCD pool (1) or one per block of the launch (0)
 *   bits 12-13 jump stage: EPV_PLAN_JUMPS_FUSED (inside the fused kernel), _SEGMENTS (epv_seg_search_kernel +
 *              epv_seg_assemble_kernel + epv_mh_jumps_kernel), _ALL (epv_mh_jumps_all_kernel), _GENERAL
 *              (epv_mh_jumps_kernel alone)
 *   bits 14-15 accept stage: EPV_PLAN_ACCEPT_FUSED (inside the fused kernel), _V3 (epv_mh_accept3_kernel),
 *              _CACHE (epv_mh_accept_kernel with its LDS meta cache), _NO_CACHE (epv_mh_accept_kernel without)
 *   bit  16    the accept stage reads the listed sites (proposal kernels V2 and V3; 0 = every site of the colour)
 *   bit  17    V1: the template that marginalises unobserved leaf cells (epv_set_unobserved holds a cell;
 *              it forces V1 like bit 3 does, unless EPV_OPT_LEAF_FAST is set)
 *   bit  18    V1: the template that reads the table of leaf evidence (epv_set_leaf_evidence holds a cell;
 *              it forces V1 too, unless EPV_OPT_LEAF_FAST is set, and the mask of bit 17 rides along for the
 *              cells without evidence)
 *              Beside _V2, _V3 or _FUSED (EPV_OPT_LEAF_FAST) either bit means the leaf variant of that kernel:
 *              the instantiation that takes the table and the mask as trailing arguments.
 *   bits 20-22 fused: log2 of the sites per wave (2 .. 6 for 4, 8, 16, 32 or 64 sites: EPV_FUSED_LANES, or by
 *              launch size -- with (n + 2) / 3 + 1 lanes 64 above 65536, 32 above 32768, else 16)
 *   bit  23    the jump stage's direct variants (EPV_OPT_DIRECT_SAMPLER): epv_seg_search_direct_kernel +
 *              epv_seg_assemble_direct_kernel + epv_mh_jumps_direct_kernel under _SEGMENTS, epv_mh_jumps_direct_kernel
 *              under _GENERAL; with EPV_OPT_DIRECT_FUSED the fused kernel's direct bodies (_FUSED); never with _ALL */
enum { EPV_PLAN_V1 = 0, EPV_PLAN_V2 = 1, EPV_PLAN_V3 = 2, EPV_PLAN_FUSED = 3 };
enum { EPV_PLAN_JUMPS_FUSED = 0, EPV_PLAN_JUMPS_SEGMENTS = 1, EPV_PLAN_JUMPS_ALL = 2, EPV_PLAN_JUMPS_GENERAL = 3 };
enum { EPV_PLAN_ACCEPT_FUSED = 0, EPV_PLAN_ACCEPT_V3 = 1, EPV_PLAN_ACCEPT_CACHE = 2, EPV_PLAN_ACCEPT_NO_CACHE = 3 };
int epv_phase_plan(epv_ctx *ctx, uint32_t *word);

/* Known-answer entry for the random stream, for tests: evaluates on the device the Philox4x32-10
 * block of each of n <= 2^20 counters, counters[6 i ..] = site, sweep, branch, segment, trial, block
 * (the layout of epv_philox.h, key = seed).  out[6 i ..] = (d0, d1) three times: with the inline-asm
 * multiplies, with the plain ones, and with the plain ones called with literal zeros for the fields
 * of the counter that are zero (trial and block; segment; branch).  All three pairs equal the CPU
 * oracle's block.  This checks the two source forms of the block in a kernel of its own; it does
 * not show what the compiler makes of a call site inside the MCMC kernels -- their bit identity
 * is what the comparisons of whole runs against the oracle's parallel rung establish. */
int epv_philox_kat(epv_ctx *ctx, uint64_t seed, uint32_t n, const uint32_t *counters, double *out);

/* Known-answer entry for the arithmetic, for tests: evaluates one operation on each of n <= 2^20 items,
 * in[4 i ..] -> out[6 i ..], with the functions the kernels call (epv_math.h, epv_kernels.h,
 * epv_propose2.h).  An op's results fill the first slots of the item's six doubles, the rest are 0.
 *   where = 0  a kernel of its own, one launch, one lane per item;
 *   where = 1  the host pass of the same headers inside this library (the one the ABI glue takes its
 *              per-branch constants from).  Ops that exist on the device only return EPV_ERR_ARG.
 *   op 0  x              -> epv_exp(x), epv_log(x)
 *   op 1  x              -> nojump_bound(x)                                      (device only)
 *   op 2  len, r0, r1    -> epv_seg_matrices: P00, P11, PT00, PT10, and the no-jump bounds of len r0 and
 *                           len r1 (where = 1: the bounds are 0)
 *   op 3  u, r           -> the hold time -epv_log(1 - u) / r
 *   op 4  u, trunc, r    -> Nielsen's first jump -epv_log(1 - u trunc) / r
 *   op 5  dt, scale      -> epv_stat_fix(dt, scale), the 64-bit integer in the bits of the double
 *   op 6  u, T, r        -> 1.0 or 0.0 twice: the shortcut's test 1 - u < nojump_bound(T r), and the exact
 *                           test !(-epv_log(1 - u) / r < T) it stands in for           (device only)
 * Ops 0 and 2-5 equal the CPU oracle's parallel rung bit for bit; ops 1 and 6 are what the no-jump shortcut
 * rests on (bound <= exp(-x) with room for the rounding of the exact test).  As with epv_philox_kat, this
 * checks the functions in a kernel of their own; it does not show what the compiler makes of a call site
 * inside the MCMC kernels -- that is what the comparisons of whole runs against the oracle establish. */
int epv_math_kat(epv_ctx *ctx, uint32_t op, uint32_t where, uint32_t n, const double *in, double *out);

/* Known-answer entry for the three-way merge of a triple's jumps on one branch (the sufficient statistics
 * D[8], J[8] of the acceptance stage), for tests: n <= 2^20 items, item i = three paths of 0 .. 8 jumps.
 *   heads[i]               start states (bit 0 left, bit 1 middle, bit 2 right) | left count << 4 |
 *                          middle count << 8 | right count << 12
 *   times[25 i + 8 c + k]  jump k of column c (0 left, 1 middle, 2 right), finite; times[25 i + 24] the
 *                          branch length
 * The device lays the times out with a stride as the jump store does and runs, one lane per item,
 *   form 0  merge3 with register accumulators (what the statistics and the generic acceptance call), and
 *   form 1  merge3_sel with accumulators in LDS, the heads loaded in one predicated batch before it
 *           (what the fused small-tree acceptance calls);
 * d_out[16 i + 8 form + ctx] and j_out[16 i + 8 form + ctx] are the two results.  As with the two entries
 * above, this checks the functions in a kernel of their own; it does not show what the compiler makes of
 * a call site inside the MCMC kernels -- that is what the comparisons of whole runs against the oracle
 * establish. */
int epv_merge_kat(epv_ctx *ctx, uint32_t n, const uint32_t *heads, const double *times, double *d_out, uint32_t *j_out);

/* Known-answer entry for the trial evaluator of the end-conditioned sampler (first_draw, run_trial, scan_trials
 * and the single-trial scan of epv_kernels.h), for tests: n <= 2^16 items, item i = one segment and a first trial.
 *   items[8 i ..]  site, sweep, node (<= 4095), segment (<= 4095), first trial t0 >= 1, room (jump slots left),
 *                  start state | end state << 1 | (Nielsen's method for a state change) << 2, 0
 *   reals[6 i ..]  length T > 0, rate of state 0, rate of state 1 (each > 1e-3, T * rate <= 64),
 *                  trunc = 1 - exp(-rate of the start state * T) as the caller computed it, u0 in [0, 1) = the
 *                  first draw handed to evaluation 1, the segment's start time (added to every jump time)
 * One lane per item, 64 items to a wave in the order given, so a wave's lanes mix whatever the caller puts side
 * by side.  Five evaluations, in the form the fused colour phase inlines (plain Philox multiplies):
 *   0  the single-trial scan of trial t0     1  run_trial of trial t0 on u0, no shortcut bounds
 *   2, 3, 4  scan_trials over 1, 4, 8 trials from t0
 * w_out[20 i + 4 e ..] = outcome (0 fail, 1 ok, 2 overflow), the winning trial (t0 for e < 2),
 * its jumps, M = the most jumps of any trial evaluated;  d_out[11 i] = first_draw(t0), followed by the
 * first two stored jump times of each evaluation (0 where there is none).  The key is `seed`.  Like the entries
 * above this runs the functions in a kernel of their own, not a call site inside the MCMC kernels. */
int epv_trial_kat(epv_ctx *ctx, uint64_t seed, uint32_t n, const uint32_t *items, const double *reals, uint32_t *w_out,
                  double *d_out);

/* Known-answer entry for the direct end-conditioned sampler (run_direct of csrc/epv_direct.h), for tests:
 * n <= 2^16 items, item i = one segment.
 *   items[8 i ..]  site, sweep, node (<= 4095), segment (<= 4095), room (jump slots left; the entry caps it at 64),
 *                  start state | end state << 1, the index of the segment's first draw in its stream (0 as the
 *                  kernels have it, or an odd index up to 2^24: the draws then begin in the middle of the stream,
 *                  so that an item can cross from one trial word into the next), 0
 *   reals[4 i ..]  length T, rate of state 0, rate of state 1 (each positive and finite), the segment's start
 *                  time (finite; added to every jump time)
 * One lane per item, 64 items to a wave in the order given.  w_out[4 i ..] = outcome (1 ok, 2 overflow, 3 gave
 * up), jumps, the index after the last uniform consumed, the longest run of rounds for one jump;  d_out[8 i ..] = the first 8 jump
 * times (0 where there is none).  The key is `seed`.  Like the entries above this runs the function in a kernel
 * of its own, not a call site inside the MCMC kernels. */
int epv_direct_kat(epv_ctx *ctx, uint64_t seed, uint32_t n, const uint32_t *items, const double *reals, uint32_t *w_out,
                   double *d_out);
/* Segments the direct sampler gave up on since the context was created (each rejected its proposal). */
int epv_direct_giveups(epv_ctx *ctx, uint64_t *n_giveups);

/* Missing leaf data.  unobserved[(b-1)*n_sites + s] != 0: the leaf end state of branch b at local
 * site s is not data -- the MCMC resamples it with the history (its Felsenstein vector is (1, 1)
 * instead of the indicator of the path's end state) instead of pinning it.  The node-major layout
 * of epv_upload_paths' init_state over all local columns, halos included.  Cells of the genome's
 * two end sites are never updated, so their flags have no effect.  NULL, or no nonzero entry,
 * clears the mask: then the plan and the results are those of a context that never had one.  A
 * nonzero entry on a branch that does not end in a leaf returns EPV_ERR_ARG (internal nodes are
 * latent already); before paths are resident EPV_ERR_STATE.  The device holds one bit per (leaf,
 * site), and only while a cell is flagged.  epv_upload_paths, epv_init_paths_indep and
 * epv_forward_simulate clear the mask (new paths are new data); everything else keeps it.  While a
 * cell is flagged a colour phase takes the first proposal kernel (epv_phase_mode 0, plan bit 17), or, under
 * EPV_OPT_LEAF_FAST, the leaf variant of the kernel it would take without the mask (plan bit 17 beside it).
 * epv_unobserved_cells: the number of flagged cells.  No reference counterpart. */
int epv_set_unobserved(epv_ctx *ctx, const uint8_t *unobserved);
int epv_unobserved_cells(epv_ctx *ctx, uint64_t *n_cells);

/* Fixed sites: what genomic regions are made of (the first and the last site of every chromosome or gap-free
 * stretch).  mask[s] != 0, one byte per local column, halos included: site s is
 *   1. never changed by a colour phase -- its path, its buffer bit and the cached triple likelihoods around it are
 *      after the phase what they were before it;
 *   2. context for its neighbours like any other column;
 *   3. no centre: its triple is left out of the integer J and D of epv_run_mcmc_sums, epv_run_mcmc_counts and
 *      epv_get_sufficient_statistics;
 *   4. not counted in n_accepted.
 * The colour-phase kernels are the ones of a context without a mask: a small guard launch before and after a
 * phase keeps and restores the fixed sites of its colour, and one small launch per statistics pass takes their
 * triples off the totals.  NULL, or no nonzero entry, clears the mask: then not one launch differs from a context
 * that never had one.  A proposal is still made for a fixed site; one that overflows the capacity raises the
 * overflow counter and EPV_ERR_CAPACITY although nothing was lost (repeat with a larger capacity: same results).
 * Seven summaries count triples or runs across neighbouring sites and are not cut at fixed sites yet: window
 * statistics, epoch statistics, domain statistics, domain turnover, change tracts, spatial correlations and domain
 * maps.  While one of them is on epv_set_fixed_sites returns EPV_ERR_STATE naming it, and while a mask is held
 * their epv_set_* return EPV_ERR_STATE naming epv_set_fixed_sites.  Before paths are resident EPV_ERR_STATE.
 * What clears the mask of epv_set_unobserved clears this one (new paths); everything else keeps it
 * (epv_set_capacity, epv_set_model, epv_scale_jump_times, epv_reset, epv_put_columns, epv_set_halo).
 * epv_fixed_sites: the number of fixed sites inside the range whose acceptances n_accepted counts (the owned
 * range) -- an acceptance rate is n_accepted / (sweeps * (owned sites - that number)).  No reference counterpart. */
int epv_set_fixed_sites(epv_ctx *ctx, const uint8_t *mask /* n local columns, NULL clears */);
int epv_fixed_sites(epv_ctx *ctx, uint64_t *n_fixed_updatable);

/* Leaf evidence.  p_state1[(b-1)*n_sites + s] = r, a float32: the probability that the leaf end
 * state of branch b at local site s is 1 given that cell's observation alone, under a flat prior;
 * NaN = the cell has none.  The MCMC then starts Felsenstein pruning at that leaf from
 * (q0, q1) = (1.0 - (double)r, (double)r), not normalised, and resamples the end state with the
 * history.  r = 0 and r = 1 are data bit for bit; r = 0.5 gives the chain of an unobserved cell.
 * A NaN cell is what it is without this call: data, or unobserved where epv_set_unobserved flags
 * it; where both are given, a non-NaN r wins over the mask.  The node-major layout of
 * epv_set_unobserved over all local columns, halos included; cells of the genome's two end sites
 * are never updated, so their values have no effect.  NULL, or an array of NaN only, clears the
 * table: then the plan and the results are those of a context that never had one.  A non-NaN value
 * on a branch that does not end in a leaf, or one that is infinite or outside [0, 1], returns
 * EPV_ERR_ARG naming branch and site; before paths are resident EPV_ERR_STATE.  The device holds
 * one float32 per (leaf, site), and only while a cell is non-NaN.  What clears the mask clears the
 * table (epv_upload_paths, epv_init_paths_indep, epv_forward_simulate, another tree); everything
 * else keeps it.  While a cell holds evidence a colour phase takes the first proposal kernel
 * (epv_phase_mode 0, plan bit 18), or, under EPV_OPT_LEAF_FAST, the leaf variant of the kernel it would take
 * without the table (plan bit 18 beside it).  epv_leaf_evidence_cells: the number of non-NaN cells.  No
 * reference counterpart.
 * The two ratio modes.  The target of a site carries the leaf factor q[end state].  The default mode
 * needs nothing for it (the proposal carries the same factor and the ratio stays 1).  Under
 * EPV_OPT_REFERENCE_PROPOSAL_RATIO and EPV_OPT_SAMPLE_ROOT the reference's two sums leave
 * log q[end state] behind on either side, so the kernel adds the target's share
 * log q[new end] - log q[old end] where a leaf with evidence changes state; with it both modes walk the
 * same chain up to the rounding noise that mode always carries, ~1e-11 in the log ratio
 * (tests/test_leaf_oracle.py).
 * Precondition: a hard cell (r exactly 0 or 1) agrees with the end state of the resident path; the
 * programs enforce it, this call does not look at the paths.  A cell that contradicts its path has
 * target weight 0 where the chain stands.  Default mode: the ratio is taken as 1, the cell takes the
 * evidence's state at its site's first accepted update and keeps it.  Reference-ratio mode: the sums are
 * not finite there.  With r = 1 against state 0 the ratio is (-inf) + (+inf) = NaN and the site is never
 * updated again; with r = 0 against state 1 the sum holds log(1 - p0) with p0 = 1 up to rounding, and the
 * site is rejected (-inf, NaN) or accepted and repaired (+inf) as that rounding falls.  No NaN or
 * infinity reaches the paths, tri_llh, J or D in either mode; the GPU decides bit for bit what the
 * oracle's arithmetic decides (tests/test_leaf_matrix.py). */
int epv_set_leaf_evidence(epv_ctx *ctx, const float *p_state1);
int epv_leaf_evidence_cells(epv_ctx *ctx, uint64_t *n_cells);

/* initialize_paths_indep (src/prog/epievo_sim_pairwise.cpp:62-110) on the device, for the
 * two-node tree of one branch (epv_set_tree with n_nodes = 2 and epv_set_model first):
 * every interior site gets an independent end-conditioned path root[i] -> leaf[i] by
 * forward rejection (EndCondSampling.cpp:512-542) with the context rates read off the
 * ROOT sequence; the two end sites get at most one uniformly placed jump.  Replaces the
 * upload: afterwards the paths are resident as if epv_upload_paths had been called.
 * capacity 0 = 32 jump slots. */
int epv_init_paths_indep(epv_ctx *ctx, uint64_t n_sites, const uint8_t *root_states,
                         const uint8_t *leaf_states, uint64_t seed, uint32_t capacity);

/* epievo_sim's forward simulation (src/prog/epievo_sim.cpp:102-152, 329-352 over TripletSampler,
 * src/libepievo/TripletSampler.cpp:165-184) on the device, for the tree and model set before:
 * the root sequence (root_states, one byte per site; NULL = EpiEvoModel::sample_state_sequence,
 * EpiEvoModel.cpp:281-298, with keyed uniforms), then every branch in pre-order.  The reference
 * runs ONE sequential event chain per branch; here every interior site carries its own candidate
 * stream at the rate max_c rate_c and a candidate flips the site with probability
 * rate[context]/max rate (thinning: the same law), candidates being resolved site-parallel in
 * any order their nearest-neighbour dependencies allow (csrc/epv_forward.h).  The outcome is a
 * function of `seed` alone and equals oracle/epv_oracle.c's orc_forward_thinning bit for bit; it is
 * NOT the std::mt19937 stream of the reference (that one is restated on the host:
 * csrc/host/epv_forward.cpp, bit-identical to the linked TripletSampler).  Afterwards the
 * histories are resident as after epv_upload_paths (epv_download_paths brings them to the host;
 * node states = init ^ parity of the jump count).  capacity 0 = 16 jump slots; EPV_ERR_CAPACITY
 * when a path needs more (call again with a larger capacity: same histories). */
int epv_forward_simulate(epv_ctx *ctx, uint64_t n_sites, const uint8_t *root_states, uint64_t seed,
                         uint32_t capacity, uint64_t *total_jumps);
/* wall clock of the last epv_forward_simulate: device memory management (freeing the previous paths,
 * allocating the new ones: tens of GB at n = 1e7) and the simulation itself (root sequence, every
 * branch, the count of the jumps) */
int epv_forward_last_ms(epv_ctx *ctx, double *alloc_ms, double *simulate_ms);

/* ---- the site-independent 2-rate model of epievo_initialization (IndepSite.hpp:40-72);
 * rates = {r0, r1}; J/D laid out [(b-1)*2 + state].
 * epv_indep_expectation            expectation_sufficient_statistics (IndepSite.cpp:222-238):
 *                                  conditional means summed over ALL sites
 * epv_indep_sufficient_statistics  compute_sufficient_statistics (:266-297): per-branch
 *                                  averages of the resident paths
 * epv_indep_update_paths           update_paths_indep (:241-259): fresh end-conditioned paths
 *                                  for every site; `sweep` keys the random stream
 * epv_indep_node_posterior         p_state1[node * n_sites + s], node-major over all N nodes: the
 *                                  probability of state 1 at that node and site given all leaf data;
 *                                  the preconditions and error codes of epv_indep_expectation, and
 *                                  EPV_ERR_ARG naming the figure when the device cannot stage the
 *                                  8 * N * n_sites bytes.  No reference counterpart.
 * Leaf masks and evidence.  epv_indep_expectation, epv_indep_update_paths and epv_indep_node_posterior
 * honour the mask of epv_set_unobserved and the table of epv_set_leaf_evidence: a leaf starts the
 * upward pass from (1.0 - (double)r, (double)r) where the table holds a non-NaN r, else from (1, 1)
 * where the mask flags the cell, else from the indicator of the path's end state; a non-NaN r wins
 * over the mask.  epv_indep_update_paths then draws the end state of such a cell from its conditional
 * law with the rest of the history, and keeps every other leaf cell.  r = 0.5 equals the mask bit
 * for bit, and r = 0 or 1 agreeing with the path equals data bit for bit (so does r = -0).
 * These calls process EVERY site, the genome's two end sites included: a flag or a value at an
 * end site has its effect here, although the MCMC never updates those sites.  A context that holds
 * no flagged and no non-NaN cell runs the kernels it ran before masks existed.
 * epv_indep_sufficient_statistics counts the resident paths and reads no leaf vector. */
int epv_indep_expectation(epv_ctx *ctx, const double *rates, double *J, double *D);
int epv_indep_sufficient_statistics(epv_ctx *ctx, double *J, double *D);
int epv_indep_update_paths(epv_ctx *ctx, const double *rates, uint64_t seed, uint32_t sweep);
int epv_indep_node_posterior(epv_ctx *ctx, const double *rates, double *p_state1);

/* Site-sharded runs only: total genome length (default: global_site_offset + n_sites),
 * so that the two special cases at the genome ends (SingleSiteSampler.cpp:422,427) are
 * decided on global indices. */
int epv_set_global_length(epv_ctx *ctx, uint64_t n_global);

/* Restrict MH updates to local sites [first, last] (inclusive); default [1, n_sites-2].
 * Sites outside are read-only halo/boundary columns. */
int epv_set_update_range(epv_ctx *ctx, uint64_t first, uint64_t last);

/* Site-sharded runs with wide halos ("temporal blocking"): declare the first `left` and
 * the last `right` local columns to be copies of the neighbouring shards' edge columns
 * (0 = this side is the genome end).  Because the RNG and the colouring are keyed by
 * the GLOBAL site index, a shard can update its halo columns redundantly and obtain
 * exactly what the owner computes; every colour phase makes two more columns at each
 * internal edge stale, so a halo of H columns lasts H/2 phases (H/6 sweeps) before
 * the columns must be refreshed (epv_put_columns, then epv_set_halo again).  While
 * this mode is on, sweeps shrink their update range automatically, and J/D and the
 * accept count cover the owned columns only.  Calling it also marks the halos fresh. */
int epv_set_halo(epv_ctx *ctx, uint64_t left, uint64_t right);
/* how many more colour phases the current halos allow (UINT64_MAX when unbounded) */
int epv_halo_phases_left(epv_ctx *ctx, uint64_t *phases);

/* SingleSiteSampler::reset (SingleSiteSampler.cpp:449-475): cache the complete-data
 * log-likelihood of every interior triple. */
int epv_reset(epv_ctx *ctx);
/* the same without waiting for the device: whatever is called next on the context runs behind it */
int epv_reset_async(epv_ctx *ctx);

/* n_sweeps x single_iteration (SingleSiteSampler.cpp:538-548) under the 3-colour
 * schedule; this is also the loop epievo_sim_pairwise.cpp:267-273 spells out by hand.
 * Sweep w uses RNG sweep index sweep_base + w.  n_accepted may be NULL. */
int epv_sweep(epv_ctx *ctx, uint64_t n_sweeps, uint64_t seed, uint32_t sweep_base,
              uint64_t *n_accepted);

/* One colour phase (colour = global_site % 3) of sweep `sweep`; used by multi-GPU
 * drivers that exchange halo columns between phases. */
int epv_sweep_phase(epv_ctx *ctx, int colour, uint64_t seed, uint32_t sweep,
                    uint64_t *n_accepted);

/* SingleSiteSampler::run_mcmc (SingleSiteSampler.cpp:550-598): burn_in sweeps, then
 * batch x {sweep; get_sufficient_statistics; accumulate}.  J/D ((n_nodes-1)*8 doubles
 * each) return the batch AVERAGES as the reference does; n_accepted counts the batch
 * sweeps only (acc_rate = n_accepted / (batch*(n_sites-2))). */
int epv_run_mcmc(epv_ctx *ctx, uint64_t burn_in, uint64_t batch, uint64_t seed,
                 uint32_t sweep_base, double *J, double *D, uint64_t *n_accepted);

/* Same, but with average = 0 J/D return the SUMS over the batch sweeps: a site-sharded
 * driver adds the shards' sums (exact for J) and divides once, which reproduces the
 * unsharded averages bit-for-bit. */
int epv_run_mcmc_sums(epv_ctx *ctx, uint64_t burn_in, uint64_t batch, uint64_t seed,
                      uint32_t sweep_base, int average, double *J, double *D,
                      uint64_t *n_accepted);

/* get_sufficient_statistics, per-branch overload (ParamEstimation.cpp:92-114), over
 * the update range's triples.  The sums are EXACT integers on the device -- J as counts, every
 * dwell time of branch b as rint(dt * 2^k_b) with k_b = min(61 - e(n_global * T_b), 50 - e(T_b)),
 * e(x) the frexp exponent -- and become doubles on the host (D = integer * 2^-k_b): the result
 * does not depend on the launch shape, the number of contexts or GPUs, or any summation order,
 * and lies within 2^-41 T_b per term of the exact sum at n = 1e6 (closer than a sequential
 * fp64 sum). */
int epv_get_sufficient_statistics(epv_ctx *ctx, double *J, double *D);

/* scale_jump_times (ParamEstimation.cpp:369-380): jumps *= new/old per branch. */
int epv_scale_jump_times(epv_ctx *ctx, const double *new_branches);

/* Download the current paths (what the EM driver writes out each iteration,
 * epievo_est_params_histories.cpp:280-283).  Call epv_paths_total_jumps first to size
 * `jumps`; offsets has (n_nodes-1)*n_sites + 1 entries. */
int epv_paths_total_jumps(epv_ctx *ctx, uint64_t *total);
int epv_download_paths(epv_ctx *ctx, uint8_t *init_state, uint64_t *offsets, double *jumps);

/* the cached triple log-likelihoods (private member tri_llh of the reference class);
 * exposed for parity tests.  out has n_sites entries. */
int epv_get_tri_llh(epv_ctx *ctx, double *out);

/* Halo exchange for site-sharded runs: copy `count` whole site columns (all branches)
 * starting at local site `first` to / from a packed host buffer of
 * epv_column_bytes(ctx) bytes per column. */
uint64_t epv_column_bytes(const epv_ctx *ctx);
int epv_get_columns(epv_ctx *ctx, uint64_t first, uint64_t count, void *packed);
int epv_put_columns(epv_ctx *ctx, uint64_t first, uint64_t count, const void *packed);
/* the same with the packed columns in DEVICE memory of the context's GPU (the buffer a driver
 * hands to RCCL: include/epievo_mi355x_comm.h, or a torch tensor's storage); synchronous */
int epv_pack_columns_dev(epv_ctx *ctx, uint64_t first, uint64_t count, void *d_packed);
int epv_unpack_columns_dev(epv_ctx *ctx, uint64_t first, uint64_t count, const void *d_packed);
int epv_device_of(const epv_ctx *ctx);
/* the same between two contexts of ONE GPU (equal tree and capacity), without leaving the device */
int epv_copy_columns(epv_ctx *src, uint64_t src_first, uint64_t count, epv_ctx *dst, uint64_t dst_first);
/* ... without waiting on the host: packed on src's stream into half `slot` (0 / 1) of its staging
 * buffer, unpacked on dst's stream behind an event; what the caller launches on dst's stream next
 * (epv_reset) sees the columns.  One use of a (src, slot) pair per refresh. */
int epv_copy_columns_async(epv_ctx *src, uint64_t src_first, uint64_t count, epv_ctx *dst, uint64_t dst_first,
                           int slot);

/* ---- sharded runs (new; the reference is single-process).  Contexts that split a genome -- two or
 * three on one GPU, whose colour phases overlap on their own streams (+17 % on one MI355X), and
 * those of other GPUs -- each own a contiguous range of sites plus redundant halos.
 * epv_run_mcmc_counts is epv_run_mcmc on such a context: it writes the integer totals (see
 * epv_get_sufficient_statistics) of the context's OWNED sites per batch sweep to the host array
 * counts[w][b][16] (int64, w < batch, b < n_nodes-1: J[8] as counts, then D[8] as fixed-point
 * integers of scale 2^k_b).  A driver adds the arrays of all contexts as integers -- exact, in any
 * grouping -- and epv_counts_to_stats turns the sum into J, D (average = 1: batch averages) as
 * epv_run_mcmc_sums does, so J AND D equal the one-context run bit for bit however the genome is
 * cut.  A capacity overflow (EPV_ERR_CAPACITY) still fills counts and n_accepted.
 * epv_dev_alloc returns zero-filled device memory on the context's GPU, the buffers a driver hands
 * to RCCL (halo columns, the statistics piece of the all-gather); epv_dev_write / epv_dev_read copy
 * host memory into and out of them. */
int epv_run_mcmc_counts(epv_ctx *ctx, uint64_t burn_in, uint64_t batch, uint64_t seed, uint32_t sweep_base,
                        int64_t *counts, uint64_t *n_accepted);
int epv_counts_to_stats(epv_ctx *ctx, const int64_t *counts, uint64_t batch, int average, double *J, double *D);
int epv_dev_alloc(epv_ctx *ctx, uint64_t bytes, void **device_ptr);
int epv_dev_free(epv_ctx *ctx, void *device_ptr);
int epv_dev_write(epv_ctx *ctx, void *d_dst, const void *src, uint64_t bytes);
int epv_dev_read(epv_ctx *ctx, void *dst, const void *d_src, uint64_t bytes);

int epv_get_counters(epv_ctx *ctx, epv_counters *out);

/* ---- average history of the sampled paths (new; the reference's average_paths program,
 * average_paths.cpp:31-45, over files of sampled paths).  For P = n_points grid points
 * t_0 = 0, t_1 = bin, t_{i+1} = t_i + bin (bin = branch length / (P - 1), repeated fp64 addition)
 * a sample adds, per branch b, site s and point i, the state of the path at t_i: its init state at
 * point 0, Path::state_at_time(t_i) (init XOR the parity of the jumps < t_i) at i >= 1.  A sample is
 * the resident paths after each batch sweep of epv_run_mcmc / epv_run_mcmc_sums /
 * epv_run_mcmc_counts (not the burn-in), or one epv_accumulate_path_average call.  The counts are
 * exact integers kept on the device (4 (N-1) P bytes per site), so they do not depend on the
 * kernels, contexts or GPUs.  A context counts its owned sites plus the genome's end sites when it
 * holds them: over all contexts every site once.  Off (the default) costs nothing.
 * epv_set_path_average: n_points >= 2 allocates (checked against the free device memory first;
 *   the message gives the figure) and zeroes the counts; 0 turns averaging off and frees them.
 * epv_get_path_average: counts[(b-1)][s - first][i] (uint32) of local sites first .. first+count-1,
 *   the convention of epv_get_columns; the average is counts / samples. */
int epv_set_path_average(epv_ctx *ctx, uint32_t n_points);
int epv_reset_path_average(epv_ctx *ctx);
int epv_accumulate_path_average(epv_ctx *ctx);
int epv_path_average_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_get_path_average(epv_ctx *ctx, uint64_t first, uint64_t count, uint32_t *counts);
/* the points (0 = averaging off) and the local sites first .. first+count-1 the counts cover.  Before
 * the first sample the counts are laid out again for the sites the context counts at this moment
 * (an owned range changed by epv_set_halo / epv_set_update_range); afterwards a change of those
 * sites makes the next sample fail until epv_set_path_average is called again. */
int epv_path_average_layout(epv_ctx *ctx, uint32_t *n_points, uint64_t *first, uint64_t *count);

/* ---- posterior branch-event maps (new): where in the genome, and on which branch, the state changed.
 * A sample reads, per branch b and site s, the init state a and the number of jumps k of the resident
 * path (no jump times) and adds to six uint32 planes, with e = a XOR (k & 1) the state at the child node,
 * g = (k + (a == 0)) >> 1 the 0->1 jumps and l = k - g the 1->0 jumps:
 *   0 end1 += e          1 net_gain += (a == 0 && e == 1)    2 net_loss += (a == 1 && e == 0)
 *   3 changed += (k >= 1)    4 gains += g                    5 losses += l
 * Divided by the sample count: P(state 1 at the child node) -- the imputed state of an open leaf cell --,
 * P(0 -> 1 end to end), P(1 -> 0 end to end), P(any jump, reverted ones included), E[gains], E[losses].
 * The start state needs no plane: start1 = end1 - net_gain + net_loss; the root's state is start1 of a
 * branch below the root.  Samples, sites and lifecycle are the path average's: a sample after each batch
 * sweep of epv_run_mcmc / _sums / _counts (not the burn-in) or one epv_accumulate_branch_events call;
 * the owned sites plus the genome's end sites where the context holds them (over all contexts every site
 * once); kept over epv_reset, epv_set_model, capacity growth, epv_scale_jump_times, masks, evidence and
 * epv_sweep_phase; a site range that changes after samples were taken is EPV_ERR_STATE.  There is no
 * grid, so branch lengths do not matter.  Exact integers: they depend on no kernel path, context or GPU.
 * Either, both or neither of the two accumulators may be on; off (the default) allocates and launches
 * nothing.  J, D, accept counts, paths, tri_llh and the plan word do not depend on it.
 * epv_set_branch_events: on != 0 allocates 24 (N-1) bytes per counted site (checked against the free
 *   device memory first; the message gives the figure) and zeroes the planes; 0 frees them.
 * A path holds at most 2047 jumps, so g <= 1024: the planes take 2^21 samples; a sample (or a run whose
 *   batch would pass that) beyond is EPV_ERR_STATE.  epv_branch_events_set_samples overwrites the sample
 *   count and nothing else (a hook for testing that cap).
 * epv_branch_events_layout: the local sites first .. first+count-1 the planes cover (0, 0 when off).
 * epv_get_branch_events: planes[p][b-1][s - first] (uint32) of local sites first .. first+count-1.
 * epv_get_branch_event_windows: sums[p][b-1][w - first_window] (uint64) = the planes summed over window
 *   w = GLOBAL sites [w W, (w+1) W), for n_windows windows from first_window; this context's contribution
 *   only, zero where it counts no site, so the contributions of contexts, shards and GPUs add up to the
 *   one-context result.  W = 1 gives the per-site planes, a W beyond the genome one window. */
int epv_set_branch_events(epv_ctx *ctx, int on);
int epv_reset_branch_events(epv_ctx *ctx);
int epv_accumulate_branch_events(epv_ctx *ctx);
int epv_branch_events_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_branch_events_set_samples(epv_ctx *ctx, uint64_t n_samples);
int epv_branch_events_layout(epv_ctx *ctx, uint64_t *first, uint64_t *count);
int epv_get_branch_events(epv_ctx *ctx, uint64_t first, uint64_t count, uint32_t *planes);
int epv_get_branch_event_windows(epv_ctx *ctx, uint64_t W, uint64_t first_window, uint64_t n_windows,
                                 uint64_t *sums);

/* ---- regional sufficient statistics (new): J and D per genomic window, the numbers a regional rate is
 * made of (jumps divided by dwell time, per neighbour context).  Window w = GLOBAL sites [w W, (w+1) W),
 * n_win = ceil(n_global / W).  A sample adds, per window and branch, the 16 exact integers of the
 * statistics -- J[8] as counts, D[8] as rint(dt 2^k_b) -- of the triples whose centre site lies in the
 * window, is interior (global 1 .. n_global-2) and is owned by the context (the range of the statistics,
 * not the path average's: the genome's end sites centre no triple).  The sums are 64-bit integers; added
 * over all windows (and all contexts of a genome) they equal, bit for bit, the sum over the batch sweeps
 * of the counts epv_run_mcmc_counts returns.  Samples and lifecycle are the branch events': a sample after
 * each batch sweep of epv_run_mcmc / _sums / _counts (not the burn-in) or one epv_accumulate_window_stats
 * call; kept over epv_reset, epv_set_model, capacity growth, masks, evidence and epv_sweep_phase; a site
 * range that changes after samples were taken is EPV_ERR_STATE.  k_b depends on the branch lengths and on
 * n_global: the accumulator remembers the scales of its first sample, and if they differ later (after
 * epv_scale_jump_times, another tree or epv_set_global_length) a sample or run is EPV_ERR_STATE until
 * epv_reset_window_stats.  Off (the default) allocates and launches nothing; J, D, accept counts, paths,
 * tri_llh and the plan word do not depend on it.
 * epv_set_window_stats: W >= 1 (clamped to n_global) allocates 128 (N-1) bytes per local window -- a
 *   window that meets the owned sites -- checked against the free device memory first (the message gives
 *   the figure), and zeroes them; W = 0 frees them.
 * Cap: a site adds at most q_b = rint(T_b 2^k_b) + 3072 to a branch's D per sample, so a sample, or a run
 *   whose batch would get there, is EPV_ERR_STATE when (samples + batch) min(W, owned sites) max_b q_b
 *   >= 2^63 (a run is refused before its first sweep; the message names W and the most samples that
 *   fit).  epv_window_stats_set_samples (a test hook) overwrites the sample count; the accumulator is left
 *   as it is.  With it go the remembered scales: a count above 0 on an accumulator without samples
 *   remembers the scales of now, as if the samples had been taken with them, and a count of 0 forgets them.
 * epv_window_stats_scale_exps: k[b-1] = k_b of the accumulator's D integers for the N-1 non-root nodes: the
 *   scales its first sample was taken with, or, while it holds no sample, the context's current ones.
 * epv_window_stats_layout: W as clamped and the global windows first_window .. +n_windows-1 this context
 *   holds (0, 0, 0 when off).
 * epv_get_window_stats: counts[w - first_window][b-1][16] (int64, J then D) for n_windows windows from
 *   first_window: this context's contribution, zero elsewhere, so contexts, shards and GPUs add up to
 *   the one-context result.
 * epv_window_counts_to_stats: J[w][b-1][8] = count / samples, D[w][b-1][8] = integer 2^-k_b / samples with
 *   the context's current scales. */
int epv_set_window_stats(epv_ctx *ctx, uint64_t W);
int epv_reset_window_stats(epv_ctx *ctx);
int epv_accumulate_window_stats(epv_ctx *ctx);
int epv_window_stats_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_window_stats_set_samples(epv_ctx *ctx, uint64_t n_samples);
int epv_window_stats_scale_exps(epv_ctx *ctx, int *k);
int epv_window_stats_layout(epv_ctx *ctx, uint64_t *W, uint64_t *first_window, uint64_t *n_windows);
int epv_get_window_stats(epv_ctx *ctx, uint64_t first_window, uint64_t n_windows, int64_t *counts);
int epv_window_counts_to_stats(epv_ctx *ctx, const int64_t *counts, uint64_t n_windows, uint64_t samples,
                               double *J, double *D);

/* ---- lineage origin maps (new): on which branch the state a leaf shows at a site arose, and how long it
 * has been held.  A joint property of the lineage from a leaf to the root, which the per-branch planes of
 * the branch events cannot give.
 * Leaves: the nodes v >= 1 with subtree_sizes[v] == 1, in node order.  The lineage of leaf l is v_0 = l,
 * v_1 = parent(v_0), ..., v_{d-1} (the child of the root; d = the leaf's depth).  Leaf l owns d + 1 consecutive
 * rows: rows 0 .. d-1 belong to the branches v_0 .. v_{d-1}, row d is the ROOT ROW (no jump on the lineage:
 * the state is as old as the root, its age censored at the leaf's depth).  R = sum over leaves of (d + 1).
 * One sample, per leaf l and counted site s: i* = the smallest i with a jump on branch v_i at s;
 *   origin[row(l, i*)][s] += 1,  age[l][s] += sum_{i < i*} fixT[v_i] + fix(T_{v_i*} - t_last)
 * (t_last = the last jump of branch v_i* at s), or without any jump origin[row(l, d)][s] += 1 and
 * age[l][s] += sum_{i < d} fixT[v_i].  Fixed point: H = the largest fp64 sum T_{v_0} + T_{v_1} + ... over the
 * leaves, k = 40 - e(H) (e = the frexp exponent; clamped to +-1000; 0 if H is not positive and finite),
 * fixT[v] = llrint(ldexp(T_v, k)), fix(x) = x 2^k rounded to nearest even.  All sums are integers: they depend
 * on no kernel path, context or GPU.  origin / samples is the posterior over the origin branch per leaf and
 * site, age 2^-k / samples the posterior mean age of the leaf's state in branch-length units.
 * Samples, sites and lifecycle are the branch events': a sample after each batch sweep of epv_run_mcmc /
 * _sums / _counts or one epv_accumulate_lineage_origins call; kept over epv_reset, epv_set_model, capacity
 * growth, masks, evidence and epv_sweep_phase; a changed site range lays the maps out again before the first
 * sample and is EPV_ERR_STATE after it.  The maps remember the tree, k and fixT of their first sample: after
 * epv_scale_jump_times or another epv_set_tree that changes any of them, a sample or a run is EPV_ERR_STATE
 * until epv_reset_lineage_origins (before the first sample the tables just follow).  At most 2^21 samples
 * (the branch events' cap, checked before any sweep of a run); a sample adds at most 2^40 + d to an age, so
 * the ages then stay below 2^62.
 * J, D, accept counts, paths, tri_llh and the plan word do not depend on the maps.
 * epv_set_lineage_origins: on != 0 allocates 4 R + 8 L bytes per counted site (checked against the free
 *   device memory first) and zeroes them; 0 frees everything.  A layout that fails leaves the maps off.
 * epv_lineage_origins_set_samples overwrites the sample count and nothing else (a hook for testing the cap).
 * epv_lineage_origins_layout: leaves L, rows R and the local sites first .. first+count-1 (zeros when off).
 * epv_lineage_origin_rows: per row the leaf node and the branch node (0 for a root row), R entries each.
 * epv_lineage_origins_scale_exp: k (of the first sample once there is one).
 * epv_get_lineage_origins: origin[r][s - first] (uint32, R rows) and age[l][s - first] (uint64, L rows).
 * epv_get_lineage_origin_windows: out[r][w - first_window] (uint64) for the R origin rows, then
 *   out[R + l][w - first_window] for the L age rows, summed over window w = GLOBAL sites [w W, (w+1) W): this
 *   context's contribution, zero where it counts no site, so contexts, shards and GPUs add up.  An age sum
 *   that passes 64 bits is EPV_ERR_ARG (narrower windows); callers that add contexts must check their own sums
 *   the same way (the ages come to the host in pieces of sites and are added there). */
int epv_set_lineage_origins(epv_ctx *ctx, int on);
int epv_reset_lineage_origins(epv_ctx *ctx);
int epv_accumulate_lineage_origins(epv_ctx *ctx);
int epv_lineage_origins_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_lineage_origins_set_samples(epv_ctx *ctx, uint64_t n_samples);
int epv_lineage_origins_layout(epv_ctx *ctx, uint32_t *n_leaves, uint32_t *n_rows, uint64_t *first, uint64_t *count);
int epv_lineage_origin_rows(epv_ctx *ctx, uint32_t *leaf_node, uint32_t *branch_node);
int epv_lineage_origins_scale_exp(epv_ctx *ctx, int *k);
int epv_get_lineage_origins(epv_ctx *ctx, uint64_t first, uint64_t count, uint32_t *origin, uint64_t *age);
int epv_get_lineage_origin_windows(epv_ctx *ctx, uint64_t W, uint64_t first_window, uint64_t n_windows,
                                   uint64_t *out);

/* ---- domain size spectra (new): the posterior spectrum of run lengths of every node's state along the
 * genome, for all N nodes (root and leaves included) and both states.  The first accumulator that is joint
 * along the genome: no per-site posterior can give it.  Counted as exact integers after every batch sweep; the
 * result depends on no kernel path, context, shard or GPU.
 * Node states of one sample: x_v[s] = a XOR (k & 1) for v >= 1 (a = init state, k = jumps of branch v at site s;
 * the branch events' e), x_0[s] = the init state of the branch of the root's lowest-numbered child.  No jump
 * time is read.
 * Runs over a stretch of sites [lo, lo + cnt): an END is a position p with p + 1 < cnt and x[p] != x[p + 1]; the
 * run that ends at p has length p - p' (p' = the previous end) and state x[p].
 * Bins: EPV_DOM_BINS = 128.  bin(l) = l for l < 16; otherwise, e = floor(log2 l), bin(l) = 16 + 4 (e - 4) +
 * ((l >> (e - 2)) & 3): exact up to 15, then four bins per octave; l < 2^32, the last bin is 127, bin 0 is never
 * used.  Bin b >= 16 holds lo = (4 + q) << (e - 2) .. lo + (1 << (e - 2)) - 1, e = 4 + (b - 16) / 4, q = (b - 16) % 4.
 * A context keeps a PART, what its stretch of counted sites contributes:
 *   hist[N][2][128] uint64   runs that end at an end and start after an earlier end, summed over the samples
 *   len_sum[N][2]   uint64   their lengths
 *   edge[sample][N][2] uint64  the two runs the stretch cannot close: [0] from its first site to its first end,
 *     [1] from its last end to its last site; bits 0-61 the length, bit 63 the state, bit 62 WHOLE (no end at
 *     all: both records equal, the length is cnt).  A stretch of no sites has both records 0.
 * Adjacent parts merge, in genome order, to the part of their union, and a part is closed to the result by
 * binning its first and last records (a whole record once): epvh_domain_parts_merge and epvh_domain_part_close
 * (libepv_host.so).  The runs at the genome's two ends count with the length the genome leaves them.
 * Samples, sites and lifecycle are the branch events': a sample after each batch sweep of epv_run_mcmc /
 * _sums / _counts or one epv_accumulate_domain_stats call; kept over epv_reset, epv_set_model, capacity growth,
 * epv_scale_jump_times, masks, evidence and epv_sweep_phase; a changed site range or tree lays the part out
 * again before the first sample and is EPV_ERR_STATE after it.  Off by default: nothing allocated, nothing
 * launched.  J, D, accept counts, paths, tri_llh and the plan word do not depend on it.
 * epv_set_domain_stats: max_samples >= 1 (at most 2^21) allocates hist, len_sum, 8 N ceil(cnt / 64) bytes of
 *   scratch and 16 N max_samples bytes of edge records (checked against the free device memory first) and zeroes
 *   them; 0 frees everything.  A sample beyond max_samples is EPV_ERR_STATE, and so is a run whose batch would
 *   pass it, refused before its first sweep.
 * epv_domain_stats_layout: nodes N, bins, the local sites first .. first+count-1 and the sites one block of the
 *   runs kernel covers (zeros when off).
 * epv_get_domain_stats: the context's part, unclosed; edges holds [samples][N][2]. */
int epv_set_domain_stats(epv_ctx *ctx, uint64_t max_samples);
int epv_reset_domain_stats(epv_ctx *ctx);
int epv_accumulate_domain_stats(epv_ctx *ctx);
int epv_domain_stats_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_domain_stats_layout(epv_ctx *ctx, uint32_t *n_nodes, uint32_t *n_bins, uint64_t *first, uint64_t *count,
                            uint64_t *chunk_sites);
int epv_get_domain_stats(epv_ctx *ctx, uint64_t *hist, uint64_t *len_sum, uint64_t *edges);

/* ---- change patterns (new): what happened ACROSS the branches of the tree at one site -- conserved by descent,
 * one clean change on one branch, the same change on several branches, a clade untouched while the rest of the
 * tree moved.  Joint over the branches of one sampled history, which the per-branch planes of the branch events
 * cannot give.  A sample reads, per site s and branch b (child node v = b + 1 in pre-order), the init state a_b
 * and the number of jumps k_b of the resident path (no jump times), and the tree's subtree_sizes.  Per site:
 *   c  = branches with k_b >= 1                      K  = sum of k_b
 *   ng = branches with a_b == 0 and k_b odd (a net gain)   nl = branches with a_b == 1 and k_b odd (a net loss)
 *   S_v = sum of k over the branches strictly below v (nodes v+1 .. v+subtree_sizes[v]-1) for every internal
 *         non-root node v (subtree_sizes[v] > 1, v >= 1); I = the number of such nodes
 * and the sample adds at most 1 to each of R = 12 + 2 (N-1) + I uint32 rows [R][sites]:
 *   0..5  jumps_1 .. jumps_6   K == h                  6  jumps_7plus    K >= 7
 *   7  one_branch      c == 1                          8  parallel_gain  ng >= 2
 *   9  parallel_loss   nl >= 2                         10 gain_and_loss  ng >= 1 and nl >= 1
 *   11 reverted_only   c >= 1 and ng == nl == 0 (every node shows the root's state, yet not by descent)
 *   12 + (b-1)          sole_gain[b]    c == 1, the changed branch is b, and it nets a gain
 *   12 + (N-1) + (b-1)  sole_loss[b]    the same for a net loss
 *   12 + 2 (N-1) + j    clade_changed[j]   S_v >= 1, v the j-th internal non-root node in pre-order
 * There is no dense row: P(conserved by descent) = 1 - (rows 0..6) / samples, P(the clade below v identical by
 * descent to v) = 1 - clade_changed / samples; a site without a jump on the tree writes nothing.  Which state a
 * conserved site holds is the branch events' end1.
 * Samples, sites and lifecycle are the branch events': a sample after each batch sweep of epv_run_mcmc / _sums /
 * _counts (not the burn-in) or one epv_accumulate_change_patterns call; the owned sites plus the genome's end
 * sites where the context holds them (over all contexts every site once); kept over epv_reset, epv_set_model,
 * capacity growth, epv_scale_jump_times, masks, evidence and epv_sweep_phase; a changed site range or tree lays
 * the rows out again before the first sample and is EPV_ERR_STATE after it.  An increment is at most 1 per
 * sample, so, as for the path average, no cap is kept.  Exact integers: they depend on no kernel path, context
 * or GPU.  Off (the default) allocates and launches nothing; J, D, accept counts, paths, tri_llh and the plan
 * word do not depend on it.
 * epv_set_change_patterns: on != 0 allocates 4 R bytes per counted site (checked against the free device memory
 *   first; the message gives the figure) and zeroes the rows; 0 frees them.
 * epv_change_patterns_layout: rows R, clades I, clade_node[j] = the node v of clade row j (I <= N-2 entries; may
 *   be null) and the local sites first .. first+count-1 the rows cover (zeros when off).
 * epv_get_change_patterns: rows[r][s - first] (uint32) of local sites first .. first+count-1.
 * epv_get_change_pattern_windows: sums[r][w - first_window] (uint64) = the rows summed over window w = GLOBAL
 *   sites [w W, (w+1) W), for n_windows windows from first_window; this context's contribution only, zero where
 *   it counts no site, so contexts, shards and GPUs add up to the one-context result.  W = 1 gives the per-site
 *   rows, a W beyond the genome one window. */
int epv_set_change_patterns(epv_ctx *ctx, int on);
int epv_reset_change_patterns(epv_ctx *ctx);
int epv_accumulate_change_patterns(epv_ctx *ctx);
int epv_change_patterns_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_change_patterns_layout(epv_ctx *ctx, uint32_t *n_rows, uint32_t *n_clades, uint32_t *clade_node,
                               uint64_t *first, uint64_t *count);
int epv_get_change_patterns(epv_ctx *ctx, uint64_t first, uint64_t count, uint32_t *rows);
int epv_get_change_pattern_windows(epv_ctx *ctx, uint64_t W, uint64_t first_window, uint64_t n_windows,
                                   uint64_t *sums);

/* ---- domain turnover (new): which domains (runs of consecutive sites in state 1) arose or died on which
 * branch, how large they were, and where two domains merged or one split.  Joint along the genome and across the
 * two ends of a branch: neither the domain size spectra (no link from a child's domains to its parent's), the
 * branch events (per site) nor the change patterns (one site) can give it.
 * One sample reads, per branch b (child node v = b + 1) and site s, the init state a and the jump count k of the
 * resident path (no jump time): e = a XOR (k & 1) is the state at the child node, c = k & 1 the net change.
 * Rows: R = 2 B.  Row 2 b is the START row, X = a (the parent's state as this branch sees it); row 2 b + 1 is the
 * END row, X = e.  Runs over a stretch [lo, lo + cnt) are those of the domain size spectra: an END is a position
 * p with p + 1 < cnt and X[p] != X[p + 1]; the run that ends at p has length p - p' and state X[p].
 * A run is KEPT (flag 1) iff at least one of its sites has c == 0, and TURNED OVER (flag 0) iff every site of it
 * has a net change on the branch.  Turned over: end row, state 1 = a domain BORN on the branch; start row, state
 * 1 = a parent domain that DIED; start row, state 0 = a parent gap FILLED (its flanking domains merged); end row,
 * state 0 = a gap OPENED (a domain split or was hollowed).  Kept runs are the domains and gaps that hold at
 * least one inherited site.
 * Bins: those of the domain size spectra (EPV_DOM_BINS = 128).  A context keeps a PART:
 *   hist[R][2 state][2 kept][128] uint64, len_sum[R][2][2] uint64   the runs closed inside the stretch
 *   edge[sample][R][2] uint64  the two runs the stretch cannot close: bits 0-60 the length, bit 61 KEPT, bit 62
 *     WHOLE, bit 63 the state.  A stretch of no sites has both records 0.
 * Merge and close are the domain size spectra's with one addition: a run joined from pieces is kept iff any piece
 * is kept (epvh_turnover_parts_merge, epvh_turnover_part_close in libepv_host.so).  After close, len_sum over
 * state and kept adds up to samples x sites for every row.  Where every child starts in its parent's end state
 * (the sampler's paths), the end row of b summed over kept is the domain part of node v, the start row that of
 * node parent(v), and the edge records match after clearing bit 61.
 * Samples, sites and lifecycle are the domain size spectra's; a changed site range or number of branches lays
 * the part out again before the first sample and is EPV_ERR_STATE after it.  Off by default: nothing allocated,
 * nothing launched.  J, D, accept counts, paths, tri_llh and the plan word do not depend on it.
 * epv_set_domain_turnover: max_samples >= 1 (at most 2^21) allocates hist, len_sum, 8 R ceil(cnt / 64) bytes of
 *   scratch and 16 R max_samples bytes of edge records (checked against the free device memory first; the message
 *   gives the figure) and zeroes them; 0 frees everything.  A sample beyond max_samples is EPV_ERR_STATE, and so
 *   is a run whose batch would pass it, refused before its first sweep.  At most 2^32 - 1 sites per context.
 * epv_domain_turnover_layout: rows R, bins, the local sites first .. first+count-1 and the sites one block of the
 *   runs kernel covers (zeros when off).
 * epv_get_domain_turnover: the context's part, unclosed; edges holds [samples][R][2]. */
int epv_set_domain_turnover(epv_ctx *ctx, uint64_t max_samples);
int epv_reset_domain_turnover(epv_ctx *ctx);
int epv_accumulate_domain_turnover(epv_ctx *ctx);
int epv_domain_turnover_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_domain_turnover_layout(epv_ctx *ctx, uint32_t *n_rows, uint32_t *n_bins, uint64_t *first, uint64_t *count,
                               uint64_t *chunk_sites);
int epv_get_domain_turnover(epv_ctx *ctx, uint64_t *hist, uint64_t *len_sum, uint64_t *edges);

/* ---- spatial correlations (new): two-point counts of node states and branch changes along the genome.  For a
 * 0/1 row X over a stretch of sites and a lag d, n11[d] is the number of site pairs (p, p + d) inside the stretch
 * with X[p] = X[p + d] = 1: whether sites 5, 50 or 500 apart still agree more often than chance, and whether the
 * changes on a branch arrive in clusters.  Neither the domain layers (a run ends at the first disagreement) nor
 * the per-site layers can give it.
 * One sample reads, per branch b (child node v = b + 1) and site, the init state a and the jump count k of the
 * resident path (no jump time).  Rows: R = N + B.  Row v < N is the state of node v as the domain size spectra
 * define it (x_0 = a of the branch of the root's lowest-numbered child, x_v = a XOR (k & 1)); row N + b is the net
 * change on branch b, k & 1.
 * With L = max_lag, 1 <= L <= min(1024, cnt), a context keeps a PART over its cnt sites (those of the path
 * average):
 *   n11[R][L + 1] uint64   summed over the samples; n11[r][0] counts the ones of the row
 *   edge[sample][R][2][LW] uint64, LW = ceil(L / 64)   record 0 (head): bit j = X_r[j]; record 1 (tail): bit j =
 *     X_r[cnt - L + j]; j < L, the bits beyond L in the last word are zero
 * Merge of a part A left of a part B (same samples, L and R, both of at least L sites): n11 = A.n11 + B.n11 + the
 * pairs that cross, cross[r][d] = #{k < d : tailA[L - d + k] = headB[k] = 1} summed over the samples; the head is
 * A's, the tail B's.  Close, for a part over the whole genome of n sites: left1[r][d] = n11[r][0] - the ones among
 * the last d sites (the ones at the left site of a pair), right1[r][d] = n11[r][0] - the ones among the first d
 * sites, pairs[d] = samples (n - d); the 2 x 2 table of (X[p], X[p + d]) follows (epvh_corr_parts_merge,
 * epvh_corr_part_close in libepv_host.so).
 * A context that counts fewer than max_lag sites is EPV_ERR_ARG (the message gives both figures), when the layer is
 * set or, for a range that changed since, before the first sweep of a run: a pair never spans three parts.
 * Samples, sites and lifecycle are the domain turnover's; a changed site range, number of nodes or first child of
 * the root lays the part out again before the first sample and is EPV_ERR_STATE after it.  Off by default:
 * nothing allocated, nothing launched.  J, D, accept counts, paths, tri_llh and the plan word do not depend on it.
 * epv_set_spatial_correlation: max_lag >= 1 (at most 1024) and max_samples >= 1 (at most 2^21) allocate
 *   8 R (L + 1) bytes of counts, 8 R ceil(cnt / 64) bytes of scratch and 16 R LW max_samples bytes of edge records
 *   (checked against the free device memory first; the message gives the figure) and zero them; max_lag = 0 frees
 *   everything.  A sample beyond max_samples is EPV_ERR_STATE, and so is a run whose batch would pass it, refused
 *   before its first sweep.  At most 2^32 - 1 sites per context.
 * epv_spatial_correlation_layout: rows R, max_lag, the local sites first .. first+count-1 and the sites one block
 *   of the count kernel covers (zeros when off).
 * epv_get_spatial_correlation: the context's part, unclosed; edges holds [samples][R][2][LW]. */
int epv_set_spatial_correlation(epv_ctx *ctx, uint32_t max_lag, uint64_t max_samples);
int epv_reset_spatial_correlation(epv_ctx *ctx);
int epv_accumulate_spatial_correlation(epv_ctx *ctx);
int epv_spatial_correlation_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_spatial_correlation_layout(epv_ctx *ctx, uint32_t *n_rows, uint32_t *max_lag, uint64_t *first, uint64_t *count,
                                   uint64_t *chunk_sites);
int epv_get_spatial_correlation(epv_ctx *ctx, uint64_t *n11, uint64_t *edges);

/* ---- chain mixing diagnostics (new): whether the means above can be trusted.  Per site of the sites the path
 * average counts, over the samples: moved = linked sample pairs (t - 1, t) whose whole history on the tree differs
 * (every branch's init state, jump count and the bit pattern of every jump time; content, not the buffer flag, so
 * an accepted proposal identical to the path is no move); with x_t the site's jumps over all branches, S1 = sum
 * x_t, S2 = sum x_t^2 and C_k = sum x_t x_{t-k} over linked pairs at lag k = 1 .. K = max_lag <= 16.  All exact
 * integers, independent of context, shard, GPU and kernel path.  Histories are compared through a 64-bit
 * fingerprint per site: a collision (2^-64) undercounts one move.
 * A RUN is a sequence of samples each linked to its predecessor.  epv_run_mcmc*: the state after burn-in opens a
 * run (its fingerprint is kept; it is no sample and enters no sum), each of the batch samples is linked to the one
 * before it, and the run closes when the call ends: a call adds batch to samples and to moved_pairs and
 * max(0, batch - k) to pairs[k].  epv_accumulate_mixing: the sample is linked if and only if a run is open and
 * exactly one sweep has run since its last sample; otherwise it opens a new run (counted in samples, S1 and S2,
 * linked to nothing).  epv_upload_paths (and whatever else replaces the paths), epv_scale_jump_times and
 * epv_reset_mixing close the run.
 * epv_set_mixing: max_lag 1 .. 16 allocates 28 + 12 max_lag bytes per counted site (checked against the free
 *   device memory first) and zeroes them; 0 frees everything; more than 16 is EPV_ERR_ARG.  samples never pass
 *   min(2^21, floor((2^64 - 1) / (B C)^2)) with C the capacity of now (no sum wraps): a further sample is
 *   EPV_ERR_STATE, and so is a run whose batch would pass it, refused before its first sweep.  A changed site range
 *   lays out again before the first sample and is EPV_ERR_STATE after it.  Off by default: nothing allocated,
 *   nothing launched.  J, D, accept counts, paths, tri_llh and the plan word do not depend on it.
 * epv_mixing_layout: the local sites first .. first+count-1 and max_lag (zeros when off).
 * epv_mixing_pairs: words[K + 2] = samples, moved_pairs, pairs[1 .. K].
 * epv_mixing_counts: moved[count] uint32 and sums[2 + K][count] uint64 (rows S1, S2, C_1 .. C_K) of the local
 *   sites first .. first+count-1.
 * epv_mixing_windows: moved summed over windows of W global sites, sums[n_windows], this context's contribution
 *   (as epv_get_branch_event_windows). */
int epv_set_mixing(epv_ctx *ctx, uint32_t max_lag);
int epv_reset_mixing(epv_ctx *ctx);
int epv_accumulate_mixing(epv_ctx *ctx);
int epv_mixing_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_mixing_layout(epv_ctx *ctx, uint64_t *first, uint64_t *count, uint32_t *max_lag);
int epv_mixing_pairs(epv_ctx *ctx, uint64_t *words);
int epv_mixing_counts(epv_ctx *ctx, uint64_t first, uint64_t count, uint32_t *moved, uint64_t *sums);
int epv_mixing_windows(epv_ctx *ctx, uint64_t W, uint64_t first_window, uint64_t n_windows, uint64_t *sums);

/* ---- domain maps (new): WHERE the domains are.  Per node v, size L_k and site p of the sites the path average
 * counts: counts[v][k][p] = the samples in which x_v[p] == state and p lies in a run of equal x_v of at least L_k
 * sites (x_v as the domain size spectra define it, from the meta words alone; a run is clipped to the stretch, and
 * at the two ends of the genome to the genome, as the spectra count them).  1 <= K <= 4 sizes, strictly increasing,
 * 1 <= L_k <= 1024; one state per enable.  counts[v][k+1][p] <= counts[v][k][p] <= samples; with L_1 = 1 row 0 is
 * the marginal of the node state.  The last layer of the chain.
 * A context keeps a PART over its cnt sites:
 *   counts[N][K][cnt] uint32, summed over the samples, runs clipped to the stretch
 *   edge[sample][N][2][EW] uint64, E = 2 (L_K - 1), EW = ceil(E / 64): record 0 (head) bit j = (x_v[j] == state),
 *     record 1 (tail) bit j = (x_v[cnt - E + j] == state); j < E, the bits beyond E in the last word are zero.  With
 *     L_K = 1 there are no records
 * Merge of a part A left of a part B (same samples, sizes and N, both of at least E sites): the counts concatenated;
 * then per sample, node and size, with m(.) the opening by L_k (erode by L_k, dilate by L_k), the cells under A's
 * tail receive m(tailA | headB) - m(tailA) and those under B's head m(tailA | headB) - m(headB), each 0 or 1 and
 * zero but in the last L_k - 1 cells of A and the first L_k - 1 of B; the head is A's, the tail B's.  No close step:
 * the part of the whole genome is the result (epvh_domain_maps_merge, epvh_domain_map_members in libepv_host.so).
 * A context that counts fewer than E sites is EPV_ERR_ARG (the message gives both figures), when the layer is set
 * or, for a range that changed since, before the first sweep of a run.
 * Samples, sites and lifecycle are the spatial correlations'; a changed site range, number of nodes or first child
 * of the root lays the part out again before the first sample and is EPV_ERR_STATE after it.  Off by default:
 * nothing allocated, nothing launched.  J, D, accept counts, paths, tri_llh and the plan word do not depend on it.
 * epv_set_domain_maps: n_sizes sizes, state 0 or 1 and max_samples >= 1 (at most 2^21) allocate 4 N K cnt bytes of
 *   counts, 8 N ceil(cnt / 64) bytes of scratch and 16 N EW max_samples bytes of edge records (checked against the
 *   free device memory first; the message gives the figure) and zero them; n_sizes = 0 frees everything.  A sample
 *   beyond max_samples is EPV_ERR_STATE, and so is a run whose batch would pass it, refused before its first sweep.
 *   At most 2^32 - 1 sites per context.
 * epv_domain_maps_layout: nodes N, K, sizes[4] (zeros beyond K), the state, the local sites first .. first+count-1
 *   and the sites one block of the membership kernel covers (zeros when off).
 * epv_get_domain_maps: the context's part, unmerged; edges holds [samples][N][2][EW]. */
int epv_set_domain_maps(epv_ctx *ctx, uint32_t n_sizes, const uint32_t *sizes, uint32_t state, uint64_t max_samples);
int epv_reset_domain_maps(epv_ctx *ctx);
int epv_accumulate_domain_maps(epv_ctx *ctx);
int epv_domain_maps_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_domain_maps_layout(epv_ctx *ctx, uint32_t *n_nodes, uint32_t *n_sizes, uint32_t *sizes, uint32_t *state,
                           uint64_t *first, uint64_t *count, uint64_t *chunk_sites);
int epv_get_domain_maps(epv_ctx *ctx, uint32_t *counts, uint64_t *edges);

/* ---- change tracts (new): what the net changes on a branch did to the domains, and how many sites each event
 * took.  Per branch b (child node b + 1) and counted site: c = k & 1 the net change, y = a XOR (k & 1) the end state
 * (a = init state, k = jumps of the branch at the site; the start state is y ^ c).  A TRACT is a maximal run of
 * sites with c = 1.  Its direction is 0 = gain (every y = 1), 1 = loss (every y = 0), 2 = mixed; its left and right
 * flanks are y of the unchanged site before and after it, 2 = none where the tract touches the genome's first or
 * last counted site.  class = direction * 9 + left * 3 + right (27 classes): a gain between flanks 0 | 0 is a domain
 * born, between 0 | 1 or 1 | 0 a domain that grew by exactly that many sites at one edge, between 1 | 1 a gap
 * filled; losses are death (0 | 0), shrinkage and a split (1 | 1).  The length goes to the bins of the domain
 * statistics (csrc/epv_domain_bin.h).  Only the 16-bit meta words are read.
 * A context keeps a PART over its cnt sites (the sites of the domain turnover):
 *   hist[B][27][128], len_sum[B][27] uint64: the tracts with an unchanged site on both sides inside the stretch,
 *     summed over the samples
 *   edge[sample][B][2] uint64: record 0 for the stretch's first site, record 1 for its last; the bits are in
 *     csrc/epv_tract_rec.h (length of the tract that holds the site, the site's y, has-gain, has-loss, the flank
 *     inside the stretch, "whole" when every site changed).  An empty stretch has both records 0
 * Merge of adjacent parts in genome order: tracts joined across a cut add their lengths and OR their direction bits,
 * take the left flank of the leftmost piece and the right flank of the rightmost; a tract that ends at a cut takes the
 * neighbour's boundary y as its flank.  Close: the tracts still open at the two ends are binned with flank 2
 * (epvh_tract_parts_merge, epvh_tract_part_close in libepv_host.so).  After close, len_sum over the classes of a
 * branch is the number of its changed sites over the samples.
 * Samples, sites and lifecycle are the domain turnover's; a changed site range or number of branches lays the part
 * out again before the first sample and is EPV_ERR_STATE after it.  Off by default: nothing allocated, nothing
 * launched.  J, D, accept counts, paths, tri_llh and the plan word do not depend on it.
 * epv_set_change_tracts: max_samples >= 1 (at most 2^21) allocates 8 B (27 x 128 + 27) bytes of counts,
 *   8 x 2 B ceil(cnt / 64) bytes of scratch and 16 B max_samples bytes of edge records (checked against the free
 *   device memory first; the message gives the figure) and zeroes them; 0 frees everything.  A sample beyond
 *   max_samples is EPV_ERR_STATE, and so is a run whose batch would pass it, refused before its first sweep.  At most
 *   2^32 - 1 sites per context.
 * epv_change_tracts_layout: branches B, classes, bins, the local sites first .. first+count-1 and the sites one block
 *   of the tract kernel covers (zeros when off).
 * epv_get_change_tracts: the context's part, unclosed; edges holds [samples][B][2]. */
int epv_set_change_tracts(epv_ctx *ctx, uint64_t max_samples);
int epv_reset_change_tracts(epv_ctx *ctx);
int epv_accumulate_change_tracts(epv_ctx *ctx);
int epv_change_tracts_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_change_tracts_layout(epv_ctx *ctx, uint32_t *n_branches, uint32_t *n_classes, uint32_t *n_bins, uint64_t *first,
                             uint64_t *count, uint64_t *chunk_sites);
int epv_get_change_tracts(epv_ctx *ctx, uint64_t *hist, uint64_t *len_sum, uint64_t *edges);

/* ---- epoch statistics (new): J and D per branch and epoch of the branch -- WHEN inside a branch the
 * changes happened, and in which neighbour context.  The direct posterior check of rates that are constant
 * over the tree.  epv_set_epoch_stats(ctx, P), 1 <= P <= EPV_EPOCH_MAX_P (0 = off and free), keeps J[8] and
 * D[8] for every branch b and epoch p = 0 .. P-1 over the triples the whole-genome statistics count (centre
 * site interior and owned).  Everything is defined on the triple's own fixed-point clock, so the result is
 * integers only:  with the branch's scale 2^k_b and fixT_b = llrint(T_b 2^k_b) (< 2^50) the epoch edges are
 * E_p = floor(p fixT_b / P), E_P = +inf (the last epoch absorbs any overshoot), bin(c) = the largest
 * p <= P-1 with E_p <= c.  A triple's events are walked in the order and with the tie rules of the
 * whole-genome statistics, with an integer clock c from 0: an interval adds F = rint((t - prev) 2^k_b), the
 * integer those statistics add for it, and occupies [c, c + F); D[b][p][ctx] receives its overlap with
 * [E_p, E_p+1); then c += F, and a jump of the centre site at the interval's end adds 1 to
 * J[b][bin(c)][ctx before the jump].  The clock differs from real time by at most 3072 quanta (about 1e-9 of
 * a branch), and sum_p D[b][p][ctx] equals the whole-genome integer exactly: summed over the epochs the
 * closed result equals, bit for bit, the sum over the batch sweeps of the counts epv_run_mcmc_counts
 * returns.  Samples and lifecycle are the window statistics': a sample after each batch sweep of epv_run_mcmc
 * / _sums / _counts (not the burn-in) or one epv_accumulate_epoch_stats call; kept over epv_reset,
 * epv_set_model, capacity growth, masks, evidence and epv_sweep_phase; the scales of the first sample are
 * remembered and a sample under other scales is EPV_ERR_STATE until epv_reset_epoch_stats; a failed launch
 * counts no sample.  Off (the default) allocates and launches nothing; J, D, accept counts, paths, tri_llh
 * and the plan word do not depend on it.
 * The context keeps a RAW difference form that is linear -- contexts, shards and GPUs of a genome add their
 * raw parts word by word as integers -- and is closed once on the host (epvh_epoch_close, libepv_host):
 * raw[b][p][32] uint64 = J[8], lo[8], hi[8], cov[8]; part = lo + 2^32 hi holds the pieces of the two end
 * bins of every interval, cov (two's complement) +1 where an interval starts to cover whole bins and -1
 * where that ends; D[p] = part[p] + (E_p+1 - E_p) sum_{q <= p} cov[q].  256 bytes per branch and epoch.
 * Cap: every raw word receives at most one addend below 2^32 per block of sites and sample, so a sample, or
 *   a run whose batch would get there, is EPV_ERR_STATE when addends + batch x blocks >= 2^32 (blocks =
 *   ceil(owned sites / sites per block), at least 256 sites per block; addends = the blocks of every sample
 *   taken so far, samples x blocks while the owned range stays; a run is refused before its first sweep).  epv_epoch_stats_set_samples (a test hook) overwrites the sample count, with the remembered
 *   scales as epv_window_stats_set_samples does.
 * epv_epoch_stats_layout: B = N-1 and P (0, 0 when off); k[b-1] = k_b and fixT[b-1] = fixT_b of the
 *   accumulator's samples (of the context's current scales while it holds none); k and fixT may be null.
 * epv_get_epoch_stats: raw[B][P][32], this context's contribution. */
#define EPV_EPOCH_MAX_P 256u
int epv_set_epoch_stats(epv_ctx *ctx, uint32_t P);
int epv_reset_epoch_stats(epv_ctx *ctx);
int epv_accumulate_epoch_stats(epv_ctx *ctx);
int epv_epoch_stats_samples(epv_ctx *ctx, uint64_t *n_samples);
int epv_epoch_stats_set_samples(epv_ctx *ctx, uint64_t n_samples);
int epv_epoch_stats_layout(epv_ctx *ctx, uint32_t *B, uint32_t *P, int *k, uint64_t *fixT);
int epv_get_epoch_stats(epv_ctx *ctx, uint64_t *raw);

/* Timing hook for bench.py: average duration (ms) of the colour-phase kernel launches
 * issued since the last call, measured with HIP events on the context's stream, and
 * how many launches that covers.  epv_set_timing(ctx, N): 0 = off, N >= 1 = events around every
 * N-th colour-phase launch (every launch costs ~4 % of a step at three contexts per GPU). */
int epv_kernel_time_ms(epv_ctx *ctx, double *avg_ms, uint64_t *n_launches);
int epv_set_timing(epv_ctx *ctx, int enabled);

#ifdef __cplusplus
}
#endif

#endif
