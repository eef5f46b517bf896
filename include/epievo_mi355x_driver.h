/* epievo_mi355x_driver.h -- flat C face of epv::SingleSiteSampler (epievo_amd/csrc/host/epv_sampler.hpp),
 * the C++ mirror of the reference's class (/root/reference/src/libepievo/SingleSiteSampler.hpp:35-81)
 * that the drop-in CLIs drive: the EM loop's E-step over every GPU of a node, RCCL linked directly
 * (libepv_rccl.so).  It exists so that programs without a C++ compiler -- bench.py, the tests --
 * run THE product driver instead of a parallel implementation of it.  -> epievo_amd/libepv_driver.so
 *
 *   epvd_create       every GPU slot in this process (device list; repeats rehearse an N-GPU run
 *                     on fewer GPUs through the loopback transport)            ncclCommInitAll
 *   epvd_create_rank  one slot per process (torchrun-style launchers); rank 0 makes the id with
 *                     epvd_unique_id and the launcher passes it around         ncclCommInitRank
 * Calls return 0 or non-zero; the text is in epvd_last_error (per thread for failed creates).
 * Paths are node-major flat as in epievo_mi355x.h; J/D are [(b-1)*8 + ctx] batch averages.
 */
#ifndef EPIEVO_MI355X_DRIVER_H
#define EPIEVO_MI355X_DRIVER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct epvd_sampler epvd_sampler;

epvd_sampler *epvd_create(uint64_t burn_in, uint64_t batch, int n_devices, const int *devices, uint32_t capacity);
int epvd_unique_id(void *id128);
epvd_sampler *epvd_create_rank(uint64_t burn_in, uint64_t batch, int device, int world, int rank,
                               const void *id128, uint32_t capacity);
void epvd_destroy(epvd_sampler *s);
const char *epvd_last_error(const epvd_sampler *s);

/* cut points of `world` slots of an n-site genome (world + 1 entries written; returns how many
 * slots the genome can feed: fewer than `world` when it is too short) */
int epvd_shard_cuts(uint64_t n_sites, int world, uint64_t burn_in, uint64_t batch, uint64_t *cuts);

/* SingleSiteSampler::reset(model, paths) with the tree of TreeHelper; n_global = 0: `paths` is the
 * whole genome (epvd_create); otherwise the owned columns of this process's slot (epvd_create_rank) */
int epvd_reset(epvd_sampler *s, const double *rates, const double *T, int n_nodes, const uint32_t *parent_ids,
               const uint32_t *subtree_sizes, const double *branches, uint64_t n_sites, const uint8_t *init_state,
               const uint64_t *offsets, const double *jumps, uint64_t n_global);
/* reset after a model change (the EM loop's second and later iterations) */
int epvd_reset_model(epvd_sampler *s, const double *rates, const double *T);
/* SingleSiteSampler::run_mcmc (SingleSiteSampler.cpp:550-598) */
int epvd_run_mcmc(epvd_sampler *s, uint64_t seed, uint64_t em_iteration, double *J, double *D, double *acc_rate);
int epvd_scale_jump_times(epvd_sampler *s, const double *new_branches, int n_nodes);
/* the resident paths (one slot per process: its owned columns): sizes first, then the copy */
int epvd_download_sizes(epvd_sampler *s, uint64_t *n_sites, uint64_t *total_jumps);
int epvd_download(epvd_sampler *s, uint8_t *init_state, uint64_t *offsets, double *jumps);

/* how the genome is laid out (tests, bench lines) */
int epvd_layout(epvd_sampler *s, char *buf, int len, int *n_slots_here, int *n_parts_here, int *uses_rccl,
                uint64_t *halo_columns);
int epvd_set_options(epvd_sampler *s, uint32_t flags);           /* EPV_OPT_* on every context, also those of later resets */
int epvd_set_timing(epvd_sampler *s, int every);                 /* epv_set_timing on every context */
int epvd_kernel_time_ms(epvd_sampler *s, double *avg_ms, uint64_t *n_launches);
int epvd_phase_mode(epvd_sampler *s, uint32_t *mode);
/* missing leaf data: epv_set_unobserved over the whole genome, unobserved[(b-1)*n_sites + s] (all n_sites
 * columns also under epvd_create_rank: each process takes its own window).  Kept across epvd_reset_model
 * and applied to the contexts of every later epvd_reset, whose genome must have n_sites columns and
 * n_nodes nodes; NULL clears */
int epvd_set_unobserved(epvd_sampler *s, uint64_t n_sites, int n_nodes, const uint8_t *unobserved);
/* leaf evidence: epv_set_leaf_evidence over the whole genome, p_state1[(b-1)*n_sites + s] (NaN = none), kept
 * and applied exactly as epvd_set_unobserved's mask is; NULL clears */
int epvd_set_leaf_evidence(epvd_sampler *s, uint64_t n_sites, int n_nodes, const float *p_state1);
/* genomic regions: the numbers of sites of the chromosomes or gap-free stretches of the whole genome, in its order,
 * each at least 3, summing to it; their end sites are held fixed (epv_set_fixed_sites, every context its window),
 * and the acceptance rate of epvd_run_mcmc is over the sites that can be updated.  Kept and applied as
 * epvd_set_unobserved's mask is; NULL or n_regions = 0 clears */
int epvd_set_regions(epvd_sampler *s, uint64_t n_regions, const uint64_t *lengths);

/* the average history of the sampled paths (epv_set_path_average on every context; 0 = off; kept
 * across epvd_reset, which starts the counts from zero), and its counts over the sites of this process
 * in genome order: sizes first (n_values = (n_nodes - 1) * sites * n_points), then the copy of
 * counts[((b-1) * sites + site) * n_points + i]; the average is counts / n_samples */
int epvd_set_path_average(epvd_sampler *s, uint32_t n_points);
int epvd_path_average_sizes(epvd_sampler *s, uint64_t *n_values, uint32_t *n_points, uint64_t *n_samples);
int epvd_download_path_average(epvd_sampler *s, uint32_t *counts);

/* posterior branch-event maps (epv_set_branch_events on every context; kept across epvd_reset, which starts
 * the planes from zero), and the six planes over the sites of this process in genome order: sizes first
 * (n_values = 6 * (n_nodes - 1) * sites), then the copy of planes[(p * (n_nodes-1) + b-1) * sites + site].
 * epvd_download_branch_event_windows: sums[(p * (n_nodes-1) + b-1) * n_windows + w] over windows of W
 * global sites, the contexts of this process added; n_windows must be ceil(genome length / W) */
int epvd_set_branch_events(epvd_sampler *s, int on);
int epvd_branch_events_sizes(epvd_sampler *s, uint64_t *n_values, uint64_t *n_samples);
int epvd_download_branch_events(epvd_sampler *s, uint32_t *planes);
int epvd_download_branch_event_windows(epvd_sampler *s, uint64_t W, uint64_t n_windows, uint64_t *sums,
                                       uint64_t *n_samples);

/* chain mixing diagnostics (epv_set_mixing on every context, max_lag = 0: off; kept across epvd_reset, which starts
 * the counts from zero).  Sizes first: the sites of this process and max_lag K; then the copy of words[K + 2]
 * (samples, moved_pairs, pairs[1 .. K]: the same on every context, else an error), moved[site] and
 * sums[r * sites + site] (rows S1, S2, C_1 .. C_K) in genome order */
int epvd_set_mixing(epvd_sampler *s, uint32_t max_lag);
int epvd_mixing_sizes(epvd_sampler *s, uint64_t *n_sites, uint32_t *max_lag);
int epvd_download_mixing(epvd_sampler *s, uint64_t *words, uint32_t *moved, uint64_t *sums);

/* regional sufficient statistics (epv_set_window_stats on every context, W = 0: off; kept across epvd_reset,
 * which starts the sums from zero).  Sizes first: W as clamped to the genome, n_windows = ceil(genome
 * length / W) and the sample count; then the copy of counts[(w * (n_nodes-1) + b-1) * 16 + c] (int64, J[8]
 * then D[8]), all slots and contexts of this process added as integers, and -- where J and D are not null
 * and samples were taken -- J, D[(w * (n_nodes-1) + b-1) * 8 + c] per sample, D in time units.  counts may
 * be null. */
int epvd_set_window_stats(epvd_sampler *s, uint64_t W);
int epvd_window_stats_sizes(epvd_sampler *s, uint64_t *W, uint64_t *n_windows, uint64_t *n_samples);
int epvd_download_window_stats(epvd_sampler *s, int64_t *counts, double *J, double *D);

/* lineage origin maps (epv_set_lineage_origins on every context; kept across epvd_reset, which starts the maps
 * from zero).  epvd_lineage_origin_rows: the leaves L, the rows R and, where the pointers are not null, per row
 * the leaf node and the branch node (0 = a leaf's root row).  epvd_lineage_origins_scale_exp: k.  The maps over
 * the sites of this process in genome order: sizes first (n_origin = R * sites, n_age = L * sites, k = the ages' scale exponent), then the copy of
 * origin[r * sites + site] and age[l * sites + site].  epvd_download_lineage_origin_windows:
 * origin[r * n_windows + w] and age[l * n_windows + w] over windows of W global sites, the slots and contexts of
 * this process added as integers (a sum beyond 64 bits is an error, not wrapped); n_windows must be
 * ceil(genome length / W) */
int epvd_set_lineage_origins(epvd_sampler *s, int on);
int epvd_reset_lineage_origins(epvd_sampler *s);
int epvd_accumulate_lineage_origins(epvd_sampler *s);
int epvd_lineage_origin_rows(epvd_sampler *s, uint32_t *n_leaves, uint32_t *n_rows, uint32_t *leaf_node,
                             uint32_t *branch_node);
int epvd_lineage_origins_scale_exp(epvd_sampler *s, int *k);
int epvd_lineage_origins_sizes(epvd_sampler *s, uint64_t *n_origin, uint64_t *n_age, int *k, uint64_t *n_samples);
int epvd_download_lineage_origins(epvd_sampler *s, uint32_t *origin, uint64_t *age);
int epvd_download_lineage_origin_windows(epvd_sampler *s, uint64_t W, uint64_t n_windows, uint64_t *origin,
                                         uint64_t *age, int *k, uint64_t *n_samples);

/* domain size spectra (epv_set_domain_stats on every context; max_samples = 0 is off; kept across epvd_reset,
 * which starts them from zero).  The part of this process: the parts of its slots and contexts merged in genome
 * order, unclosed -- sizes first (nodes N and samples S), then the copy of hist[N][2][128], len_sum[N][2] and
 * edges[S][N][2].  epvd_download_domain_stats: that part closed, into hist[n_nodes][2][128] and
 * len_sum[n_nodes][2] (n_nodes = the tree's); one slot per process: an error that names the part and the merge
 * function, because one process's stretch is not the genome */
int epvd_set_domain_stats(epvd_sampler *s, uint64_t max_samples);
int epvd_reset_domain_stats(epvd_sampler *s);
int epvd_accumulate_domain_stats(epvd_sampler *s);
int epvd_domain_part_sizes(epvd_sampler *s, uint32_t *n_nodes, uint64_t *n_samples);
int epvd_download_domain_part(epvd_sampler *s, uint64_t *hist, uint64_t *len_sum, uint64_t *edges);
int epvd_download_domain_stats(epvd_sampler *s, uint32_t n_nodes, uint64_t *hist, uint64_t *len_sum,
                               uint64_t *n_samples);

/* the turnover of domains per branch (epv_set_domain_turnover on every context; max_samples = 0 is off; kept across
 * epvd_reset, which starts it from zero).  The part of this process: the parts of its slots and contexts merged in
 * genome order, unclosed -- sizes first (rows R = 2 B and samples S), then the copy of hist[R][2][2][128],
 * len_sum[R][2][2] and edges[S][R][2].  epvd_download_turnover: that part closed, into hist[n_rows][2][2][128] and
 * len_sum[n_rows][2][2] (n_rows = twice the tree's branches); one slot per process: an error that names the part
 * and the merge function, because one process's stretch is not the genome */
int epvd_set_turnover(epvd_sampler *s, uint64_t max_samples);
int epvd_reset_turnover(epvd_sampler *s);
int epvd_accumulate_turnover(epvd_sampler *s);
int epvd_turnover_part_sizes(epvd_sampler *s, uint32_t *n_rows, uint64_t *n_samples);
int epvd_download_turnover_part(epvd_sampler *s, uint64_t *hist, uint64_t *len_sum, uint64_t *edges);
int epvd_download_turnover(epvd_sampler *s, uint32_t n_rows, uint64_t *hist, uint64_t *len_sum, uint64_t *n_samples);

/* the change tracts per branch (epv_set_change_tracts on every context; max_samples = 0 is off; kept across
 * epvd_reset, which starts them from zero).  The part of this process: the parts of its slots and contexts merged in
 * genome order, unclosed -- sizes first (branches B and samples S), then the copy of hist[B][27][128], len_sum[B][27]
 * and edges[S][B][2].  epvd_download_tracts: that part closed, into hist[n_branches][27][128] and
 * len_sum[n_branches][27] (n_branches = the tree's branches); one slot per process: an error that names the part and
 * the merge function, because one process's stretch is not the genome */
int epvd_set_tracts(epvd_sampler *s, uint64_t max_samples);
int epvd_reset_tracts(epvd_sampler *s);
int epvd_accumulate_tracts(epvd_sampler *s);
int epvd_tracts_part_sizes(epvd_sampler *s, uint32_t *n_branches, uint64_t *n_samples);
int epvd_download_tracts_part(epvd_sampler *s, uint64_t *hist, uint64_t *len_sum, uint64_t *edges);
int epvd_download_tracts(epvd_sampler *s, uint32_t n_branches, uint64_t *hist, uint64_t *len_sum, uint64_t *n_samples);

/* spatial correlations (epv_set_spatial_correlation on every context; max_lag = 0 is off; kept across epvd_reset,
 * which starts them from zero).  The part of this process: the parts of its slots and contexts merged in genome
 * order, unclosed -- sizes first (rows R = N + B, max_lag L, samples S and the sites the part covers), then the copy
 * of n11[R][L + 1] and edges[S][R][2][ceil(L / 64)].  epvd_download_corr: that part closed, into n11, left1 and
 * right1 [n_rows][max_lag + 1]; one slot per process: an error that names the part and the merge function, because
 * one process's stretch is not the genome */
int epvd_set_corr(epvd_sampler *s, uint32_t max_lag, uint64_t max_samples);
int epvd_reset_corr(epvd_sampler *s);
int epvd_accumulate_corr(epvd_sampler *s);
int epvd_corr_part_sizes(epvd_sampler *s, uint32_t *n_rows, uint32_t *max_lag, uint64_t *n_samples, uint64_t *n_sites);
int epvd_download_corr_part(epvd_sampler *s, uint64_t *n11, uint64_t *edges);
int epvd_download_corr(epvd_sampler *s, uint32_t n_rows, uint32_t max_lag, uint64_t *n11, uint64_t *left1,
                       uint64_t *right1, uint64_t *n_samples);

/* domain maps (epv_set_domain_maps on every context; n_sizes = 0 is off; kept across epvd_reset, which starts them
 * from zero).  The part of this process: the parts of its slots and contexts merged in genome order -- sizes first
 * (nodes N, sizes K, samples S and the sites the part covers), then the copy of counts[N][K][sites] (uint32) and
 * edges[S][N][2][ceil((L_K - 1) / 32)].  Of one process of several it is that process's stretch: merge the processes'
 * parts in genome order (epvh_domain_maps_merge) */
int epvd_set_dmaps(epvd_sampler *s, uint32_t n_sizes, const uint32_t *sizes, uint32_t state, uint64_t max_samples);
int epvd_reset_dmaps(epvd_sampler *s);
int epvd_accumulate_dmaps(epvd_sampler *s);
int epvd_dmaps_sizes(epvd_sampler *s, uint32_t *n_nodes, uint32_t *n_sizes, uint64_t *n_samples, uint64_t *n_sites);
int epvd_download_dmaps(epvd_sampler *s, uint32_t *counts, uint64_t *edges);

/* change patterns (epv_set_change_patterns on every context; kept across epvd_reset, which starts the rows from
 * zero), and the rows over the sites of this process in genome order: sizes first (n_rows = 12 + 2 (n_nodes-1) +
 * internal non-root nodes, n_values = n_rows * sites), then the copy of rows[r * sites + site].
 * epvd_download_change_pattern_windows: sums[r * n_windows + w] over windows of W global sites, the slots and
 * contexts of this process added; n_rows as the sizes gave it, n_windows must be ceil(genome length / W) */
int epvd_set_change_patterns(epvd_sampler *s, int on);
int epvd_change_patterns_sizes(epvd_sampler *s, uint64_t *n_values, uint32_t *n_rows, uint64_t *n_samples);
int epvd_download_change_patterns(epvd_sampler *s, uint32_t *rows);
int epvd_download_change_pattern_windows(epvd_sampler *s, uint64_t W, uint32_t n_rows, uint64_t n_windows,
                                         uint64_t *sums, uint64_t *n_samples);

/* epoch statistics (epv_set_epoch_stats on every context, P = 0: off; kept across epvd_reset, which starts
 * the sums from zero).  Sizes first: P and the sample count; then the copy of the closed counts
 * closed[((b-1) * P + p) * 24 + ..] (uint64: J[8], then D[8] as 128-bit integers, low words [8] and high words
 * [8]) -- the raw parts of all slots and contexts of this process added as integers and closed once --, of
 * k[b-1] = k_b and fixT[b-1] = fixT_b, and, where J and D are not null and samples were taken,
 * J, D[((b-1) * P + p) * 8 + c] per sample, D in time units.  closed, k and fixT may be null. */
int epvd_set_epoch_stats(epvd_sampler *s, uint32_t P);
int epvd_epoch_stats_sizes(epvd_sampler *s, uint32_t *P, uint64_t *n_samples);
int epvd_download_epoch_stats(epvd_sampler *s, uint64_t *closed, int *k, uint64_t *fixT, double *J, double *D);

#ifdef __cplusplus
}
#endif

#endif
