// epv_sampler.hpp -- host-side C++ face of the GPU sampler, shaped like the reference's
// SingleSiteSampler (/root/reference/src/libepievo/SingleSiteSampler.hpp:35-81) so that
// the EM driver reads like the reference's (epievo_est_params_histories.cpp:236-264).
// It is a wrapper over the C ABIs of include/epievo_mi355x.h (kernels) and
// include/epievo_mi355x_comm.h (RCCL); errors become std::runtime_error (the reference's mains
// catch std::exception and return EXIT_FAILURE, epievo_est_params_histories.cpp:296-299).
//
// Differences forced by the device boundary:
//  * paths live on the GPU between calls: reset(model, tree, paths) uploads them once,
//    reset(model) re-derives the cached log-likelihoods after a model change, and
//    download(paths) brings them back when the driver wants to write them;
//  * the reference threads one std::mt19937 through every call; the parallel schedule
//    uses a counter-based stream, so run_mcmc takes (seed, em_iteration) instead.
//
// Sharding (new; the reference is single-threaded).  The genome is cut into PARTS in genome
// order: G device slots (one per GPU of the node: EPV_DEVICES / the constructor's device list)
// times k contexts per GPU (EPV_CONTEXTS_PER_GPU, default 2).  Every part owns whole 256-site
// blocks plus redundant halo columns wide enough for a whole run_mcmc; the RNG and the colouring
// are keyed by the global site index, so the parts need no communication inside the E-step.
// Per EM iteration the slots exchange, device to device through RCCL,
//   (1) the edge columns of neighbouring parts before reset()          (epv_comm_exchange), and
//   (2) their integer J/D totals per batch sweep after run_mcmc()      (epv_comm_all_gather);
// integer sums do not depend on how they are grouped, so paths, J, D and the acceptance rate are
// bit-identical to the one-context run for any G and k.  A device list with
// repeats (EPV_DEVICES=0,0,0,0) rehearses an N-GPU run on a smaller box through the loopback
// transport of the exchange layer.
//
// Two ways to place the GPU slots (include/epievo_mi355x_comm.h):
//   * every slot in THIS process (the CLIs, `bench.py --gpus N` called plainly): the constructor's
//     device list, one RCCL communicator rank per slot through ncclCommInitAll;
//   * one slot per process (RankSpec; torchrun-style launchers): the process owns slot `rank` of
//     `world`, reset() takes the OWNED columns of that slot (shard_cuts tells which), the halo
//     columns arrive from the neighbouring ranks before the first reset, and the communicator
//     comes from ncclCommInitRank with an id the launcher passes around.
// Both run the same code below; the loops simply cover the slots that live here.
#ifndef EPV_SAMPLER_HPP
#define EPV_SAMPLER_HPP

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "epv_io.hpp"
#include "epv_model.hpp"

struct epv_ctx;
struct epv_comm;

namespace epv {

// "all" | "0,1,2,3" | "" (-> {0}); repeats allowed (rehearsal).  Throws on a malformed list.
std::vector<int> parse_device_list(const std::string &spec);
// the device list of the environment (EPV_DEVICES), {0} when unset
std::vector<int> devices_from_env();

// one slot of a run whose other slots live in other processes
struct RankSpec {
  int device = 0;           // the GPU of this process
  int world = 1, rank = 0;  // slots of the run, and this one's place in genome order
  unsigned char id[128] = {0};   // epv_comm_get_unique_id of rank 0, passed around by the launcher
};

class SingleSiteSampler {
public:
  SingleSiteSampler(size_t n_burn_in, size_t n_batch, int device = 0, uint32_t capacity = 0);
  SingleSiteSampler(size_t n_burn_in, size_t n_batch, const std::vector<int> &devices, uint32_t capacity = 0);
  SingleSiteSampler(size_t n_burn_in, size_t n_batch, const RankSpec &rank, uint32_t capacity = 0);
  // cut points of `world` contiguous slots of an n-site genome (multiples of 256 * row_blocks
  // sites; every slot must be able to hold its halos): world + 1 entries, or fewer when the genome
  // cannot feed that many slots
  static std::vector<uint64_t> shard_cuts(uint64_t n_sites, size_t world, size_t n_burn_in, size_t n_batch,
                                          uint32_t row_blocks = 64);
  ~SingleSiteSampler();
  SingleSiteSampler(const SingleSiteSampler &) = delete;
  SingleSiteSampler &operator=(const SingleSiteSampler &) = delete;

  // SingleSiteSampler::reset (SingleSiteSampler.cpp:449-475)
  void reset(const Model &the_model, const Tree &th, const FlatPaths &paths);
  void reset(const Model &the_model);
  // one slot per process: `owned` = the columns [cuts[rank], cuts[rank + 1]) of an n_global-site genome
  void reset(const Model &the_model, const Tree &th, const FlatPaths &owned, uint64_t n_global);

  // initialize_paths_indep (src/prog/epievo_sim_pairwise.cpp:62-110) on the device for the
  // two-node tree `th`; afterwards the paths are resident as after reset(model, th, paths)
  void init_paths_indep(const Model &the_model, const Tree &th, const std::vector<uint8_t> &root_seq,
                        const std::vector<uint8_t> &leaf_seq, uint64_t seed);

  // SingleSiteSampler::run_mcmc (:550-598).  J/D are resized to n_nodes rows of 8 (row 0
  // empty) and hold batch averages, exactly as the reference returns them.
  void run_mcmc(uint64_t seed, uint64_t em_iteration, std::vector<std::vector<double>> &J_all_sites,
                std::vector<std::vector<double>> &D_all_sites, double &acceptance_rate);

  // `n` x single_iteration (:538-548); epievo_sim_pairwise.cpp:267-273 spells this loop
  // out with Metropolis_Hastings_site.  Returns the number of accepted proposals.
  size_t sweeps(size_t n, uint64_t seed, uint32_t sweep_base);

  // scale_jump_times (ParamEstimation.cpp:369-380)
  void scale_jump_times(const std::vector<double> &new_branches);

  // the resident paths (one slot per process: the owned columns of this slot)
  void download(FlatPaths &paths);
  // average history of the sampled paths (epv_set_path_average) on every context: one sample per
  // batch sweep of run_mcmc.  n_points = 0 turns it off; the setting carries over to the contexts of a
  // later reset(model, tree, paths), which starts the counts from zero.  download_path_average:
  // counts[((b-1) * sites + site) * n_points + i] over the sites of this process in genome order (the
  // whole genome unless one slot per process), and the number of samples
  void set_path_average(uint32_t n_points);
  void download_path_average(std::vector<uint32_t> &counts, uint64_t &n_samples);
  uint32_t path_average_points() const { return pa_points_; }
  // posterior branch-event maps (epv_set_branch_events) on every context, with the path average's
  // samples and lifecycle (the setting carries over to the contexts of a later reset(model, tree, paths),
  // which starts the planes from zero).  download_branch_events: planes[(p * (n_nodes-1) + b-1) * sites +
  // site] over the sites of this process in genome order; download_branch_event_windows: sums[(p *
  // (n_nodes-1) + b-1) * n_windows + w] over windows of W global sites, all contexts of this process added
  void set_branch_events(bool on);
  bool branch_events_on() const { return bevents_; }
  uint64_t branch_event_windows(uint64_t W) const { return W ? (n_sites_ + W - 1u) / W : 0u; }   // windows of the genome
  void download_branch_events(std::vector<uint32_t> &planes, uint64_t &n_samples);
  void download_branch_event_windows(uint64_t W, std::vector<uint64_t> &sums, uint64_t &n_samples);
  // chain mixing diagnostics (epv_set_mixing) on every context, with the branch events' lifecycle (max_lag = 0:
  // off).  download_mixing: words[K + 2] = samples, moved_pairs, pairs[1 .. K] (the same on every context, else it
  // throws), moved[site] and sums[r * sites + site] (rows S1, S2, C_1 .. C_K) over the sites of this process in
  // genome order
  void enable_mixing(uint32_t max_lag);
  uint32_t mixing_max_lag() const { return mixing_lag_; }
  void download_mixing(std::vector<uint64_t> &words, std::vector<uint32_t> &moved, std::vector<uint64_t> &sums);
  // regional sufficient statistics (epv_set_window_stats) on every context: J and D per window of W global
  // sites, with the branch events' samples and lifecycle (W = 0: off).  download_window_stats:
  // counts[(w * (n_nodes-1) + b-1) * 16 + c] (J[8] then D[8] as integers) over all windows of the genome,
  // all slots and contexts of this process added; window_counts_to_stats: J, D[(w * (n_nodes-1) + b-1) * 8 + c]
  // per sample, D in time units; window_stats_scale_exps: k_b per node (index 0, the root: 0) of the
  // accumulator's D integers, from the context itself (epv_window_stats_scale_exps)
  void set_window_stats(uint64_t W);
  uint64_t window_stats_width() const { return wstat_W_ && n_sites_ ? std::min<uint64_t>(wstat_W_, n_sites_) : wstat_W_; }
  uint64_t window_stats_windows() const { const uint64_t W = window_stats_width(); return W ? (n_sites_ + W - 1u) / W : 0u; }
  void download_window_stats(std::vector<int64_t> &counts, uint64_t &W, uint64_t &n_windows, uint64_t &n_samples);
  void window_counts_to_stats(const std::vector<int64_t> &counts, uint64_t n_windows, uint64_t n_samples,
                              std::vector<double> &J, std::vector<double> &D);
  std::vector<int> window_stats_scale_exps();
  // lineage origin maps (epv_set_lineage_origins) on every context, with the branch events' samples and
  // lifecycle.  lineage_origin_rows: per row the leaf node and the branch node (0 = a leaf's root row);
  // download_lineage_origins: origin[r * sites + site] (R rows), age[l * sites + site] (L rows) over the sites
  // of this process in genome order, k = the ages' scale exponent (an age integer is a time in units of
  // 2^-k); download_lineage_origin_windows: origin[r * n_windows + w], age[l * n_windows + w] over windows of
  // W global sites, all slots and contexts of this process added as integers
  void set_lineage_origins(bool on);
  bool lineage_origins_on() const { return origins_; }
  void reset_lineage_origins();
  void accumulate_lineage_origins();
  void lineage_origin_rows(std::vector<uint32_t> &leaf_node, std::vector<uint32_t> &branch_node);
  int lineage_origins_scale_exp();   // k, the same on every context
  void download_lineage_origins(std::vector<uint32_t> &origin, std::vector<uint64_t> &age, int &k, uint64_t &n_samples);
  void download_lineage_origin_windows(uint64_t W, std::vector<uint64_t> &origin, std::vector<uint64_t> &age, int &k,
                                       uint64_t &n_samples);
  // domain size spectra (epv_set_domain_stats) on every context, with the branch events' samples and lifecycle;
  // max_samples = 0 is off.  download_domain_part: the parts of all slots and contexts of this process merged in
  // genome order (epv::domain_parts_merge), unclosed: hist [N][2][128], len_sum [N][2], edges [samples][N][2].
  // download_domain_stats: that part closed (epv::domain_part_close).  One slot per process: it throws, because
  // one process's stretch is not the genome; merge the processes' download_domain_part, then close
  void set_domain_stats(uint64_t max_samples);
  uint64_t domain_stats_max() const { return domains_max_; }
  void reset_domain_stats();
  void accumulate_domain_stats();
  void download_domain_part(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum, std::vector<uint64_t> &edges,
                            uint32_t &n_nodes, uint64_t &n_samples);
  void download_domain_stats(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum, uint32_t &n_nodes,
                             uint64_t &n_samples);
  // domain turnover (epv_set_domain_turnover) on every context, with the domain size spectra's samples and
  // lifecycle; max_samples = 0 is off.  n_rows = 2 (n_nodes-1).  download_domain_turnover_part: the parts of all
  // slots and contexts of this process merged in genome order (epv::turnover_parts_merge), unclosed: hist
  // [R][2][2][128], len_sum [R][2][2], edges [samples][R][2].  download_domain_turnover: that part closed
  // (epv::turnover_part_close).  One slot per process: it throws, as download_domain_stats does
  void set_domain_turnover(uint64_t max_samples);
  uint64_t domain_turnover_max() const { return turnover_max_; }
  void reset_domain_turnover();
  void accumulate_domain_turnover();
  void download_domain_turnover_part(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum,
                                     std::vector<uint64_t> &edges, uint32_t &n_rows, uint64_t &n_samples);
  void download_domain_turnover(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum, uint32_t &n_rows,
                                uint64_t &n_samples);
  // change tracts (epv_set_change_tracts) on every context, with the domain turnover's samples and lifecycle;
  // max_samples = 0 is off.  n_branches = n_nodes-1.  download_change_tracts_part: the parts of all slots and
  // contexts of this process merged in genome order (epv::tract_parts_merge), unclosed: hist [B][27][128], len_sum
  // [B][27], edges [samples][B][2].  download_change_tracts: that part closed (epv::tract_part_close).  One slot
  // per process: it throws, as download_domain_turnover does
  void set_change_tracts(uint64_t max_samples);
  uint64_t change_tracts_max() const { return tracts_max_; }
  void reset_change_tracts();
  void accumulate_change_tracts();
  void download_change_tracts_part(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum,
                                   std::vector<uint64_t> &edges, uint32_t &n_branches, uint64_t &n_samples);
  void download_change_tracts(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum, uint32_t &n_branches,
                              uint64_t &n_samples);
  // spatial correlations (epv_set_spatial_correlation) on every context, with the domain turnover's samples and
  // lifecycle; max_lag = 0 is off.  n_rows = 2 n_nodes - 1.  download_spatial_correlation_part: the parts of all
  // slots and contexts of this process merged in genome order (epv::corr_parts_merge), unclosed: n11 [R][L + 1],
  // edges [samples][R][2][ceil(L / 64)], over n_sites sites.  download_spatial_correlation: that part closed
  // (epv::corr_part_close) into left1 and right1 [R][L + 1].  One slot per process: it throws, as
  // download_domain_turnover does
  void set_spatial_correlation(uint32_t max_lag, uint64_t max_samples);
  uint32_t spatial_correlation_max_lag() const { return corr_lag_; }
  void reset_spatial_correlation();
  void accumulate_spatial_correlation();
  void download_spatial_correlation_part(std::vector<uint64_t> &n11, std::vector<uint64_t> &edges, uint32_t &n_rows,
                                         uint32_t &max_lag, uint64_t &n_samples, uint64_t &n_sites);
  void download_spatial_correlation(std::vector<uint64_t> &n11, std::vector<uint64_t> &left1,
                                    std::vector<uint64_t> &right1, uint32_t &n_rows, uint32_t &max_lag,
                                    uint64_t &n_samples);
  // domain maps (epv_set_domain_maps) on every context, with the spatial correlations' samples and lifecycle; no
  // sizes is off.  download_domain_maps: the parts of all slots and contexts of this process merged in genome order
  // (epv::domain_maps_merge): counts [n_nodes][sizes][n_sites], edges [samples][n_nodes][2][EW].  Of one process of
  // several it is that process's stretch: merge the processes' parts in genome order the same way
  void set_domain_maps(const std::vector<uint32_t> &sizes, uint32_t state, uint64_t max_samples);
  const std::vector<uint32_t> &domain_map_sizes() const { return dmaps_sizes_; }
  void reset_domain_maps();
  void accumulate_domain_maps();
  void download_domain_maps(std::vector<uint32_t> &counts, std::vector<uint64_t> &edges, uint32_t &n_nodes,
                            uint64_t &n_samples, uint64_t &n_sites);
  // change patterns (epv_set_change_patterns) on every context, with the branch events' samples and lifecycle.
  // n_rows = 12 + 2 (n_nodes-1) + internal non-root nodes.  download_change_patterns: rows[r * sites + site] over
  // the sites of this process in genome order; download_change_pattern_windows: sums[r * n_windows + w] over
  // windows of W global sites, all slots and contexts of this process added
  void set_change_patterns(bool on);
  bool change_patterns_on() const { return patterns_; }
  void download_change_patterns(std::vector<uint32_t> &rows, uint32_t &n_rows, uint64_t &n_samples);
  void download_change_pattern_windows(uint64_t W, std::vector<uint64_t> &sums, uint32_t &n_rows, uint64_t &n_samples);
  // epoch statistics (epv_set_epoch_stats) on every context: J and D per branch and epoch, with the window
  // statistics' samples and lifecycle (P = 0: off).  download_epoch_stats: the raw parts of all slots and
  // contexts of this process added as integers and closed once (epv::epoch_close):
  // closed[((b-1) * P + p) * 24 + ..] = J[8], D low words [8], D high words [8]; k and fixT per node (index 0,
  // the root: 0) from the context itself (epv_epoch_stats_layout); epoch_counts_to_stats: J, D[((b-1) * P + p) * 8 + c]
  // per sample, D in time units
  void set_epoch_stats(uint32_t P);
  uint32_t epoch_stats_epochs() const { return epoch_P_; }
  void download_epoch_stats(std::vector<uint64_t> &closed, std::vector<int> &k, std::vector<uint64_t> &fixT,
                            uint64_t &n_samples);
  void epoch_counts_to_stats(const std::vector<uint64_t> &closed, const std::vector<int> &k, uint64_t n_samples,
                             std::vector<double> &J, std::vector<double> &D) const;
  // EPV_OPT_* of include/epievo_mi355x.h on every context, also those a later reset(model, tree, paths)
  // makes; HIP-event timing of the colour phases
  void set_options(uint32_t flags);
  // missing leaf data (epv_set_unobserved): whole_genome[(b-1) * n_sites + s] != 0 -> the leaf end state
  // of branch b at genome site s is resampled with the history.  The whole genome also in one-slot-per-
  // process mode (each process slices its own columns).  Kept in the sampler: applied to every context
  // now if paths are resident, and to the window of every part a later reset(model, tree, paths) makes
  // (which throws when the length does not match its genome); reset(model) keeps it.  Empty = clear.
  void set_unobserved(std::vector<uint8_t> whole_genome);
  // leaf evidence (epv_set_leaf_evidence): whole_genome[(b-1) * n_sites + s] = P(leaf end state of branch b at
  // genome site s is 1 | that cell's observation), NaN = none.  Stored, sliced, re-applied and length-checked
  // exactly as set_unobserved's mask; empty or all NaN = clear.
  void set_leaf_evidence(std::vector<float> whole_genome);
  // genomic regions (chromosomes, gap-free stretches; epv_set_fixed_sites): their numbers of
  // sites in the order of the genome, each at least 3, summing to the genome.  The first and the last site of every
  // region are held fixed on every context -- each gets its window of the genome's mask, halos included -- so no
  // update and no counted triple spans a break.  Kept, windowed and re-applied as set_unobserved's mask is (a
  // reset(model, tree, paths) throws when the lengths do not sum to its genome); run_mcmc's acceptance rate is over
  // the sites that can be updated.  Empty = clear.  The seven summaries that count across neighbouring sites
  // refuse while regions are held, and regions refuse while one of them is on, with the library's message
  void set_regions(std::vector<uint64_t> lengths);
  void set_timing(int every);
  void kernel_time_ms(double &avg_ms, uint64_t &n_launches);
  uint32_t phase_mode();
  uint64_t halo_columns() const { return halo_; }

  // upload paths without touching the model (the site-independent stage has no EpiEvoModel yet).  One context;
  // set_unobserved and set_leaf_evidence work on it as after reset (a mask or table set before goes on the new
  // paths), the three indep_* calls that read leaf data honour them (include/epievo_mi355x.h), and
  // scale_jump_times keeps them
  void upload(const Tree &th, const FlatPaths &paths);
  // get_sufficient_statistics, per-branch overload (ParamEstimation.cpp:92-114), of the
  // resident paths: rows 1..n_nodes-1 of 8 contexts
  void get_sufficient_statistics(std::vector<std::vector<double>> &J, std::vector<std::vector<double>> &D);
  // the site-independent model of IndepSite.hpp:40-72; J/D flat [(b-1)*2 + state]
  void indep_expectation(const double rates[2], std::vector<double> &J, std::vector<double> &D);
  void indep_sufficient_statistics(std::vector<double> &J, std::vector<double> &D);
  void indep_update_paths(const double rates[2], uint64_t seed, uint32_t sweep);
  // epv_indep_node_posterior: p_state1[node * n_sites + s] = P(state 1 | all leaf data, mask, evidence)
  void indep_node_posterior(const double rates[2], std::vector<double> &p_state1);

  // MCMC parameter constants (public fields of the reference class)
  bool SAMPLE_ROOT;  // hard-wired false in the reference (SingleSiteSampler.cpp:441); true = EPV_OPT_SAMPLE_ROOT on
                     // every context (root states are proposed too; reference-arithmetic kernels)
  size_t burn_in;
  size_t batch;

  // capacity overflows that were absorbed by widening the device jump slots (verbose output)
  std::vector<std::string> capacity_events;

  // how the genome is laid out right now (verbose output, tests)
  size_t n_parts() const { return parts_.size(); }
  size_t n_slots() const { return slots_.size(); }
  bool uses_rccl() const;
  std::string layout() const;
  int contexts_per_gpu() const { return contexts_wanted_ > 0 ? contexts_wanted_ : (n_nodes_ - 1 <= 8 ? 3 : 2); }

private:
  struct Part {            // one context: local columns [lo, hi), owned columns [a, b) of the genome
    epv_ctx *ctx = nullptr;
    size_t slot = 0;
    uint64_t lo = 0, a = 0, b = 0, hi = 0;
  };
  struct Slot {            // one GPU of the run (or one rehearsal slot on a shared GPU) that lives here
    int device = 0;
    size_t gidx = 0;                     // its place among the run's slots
    epv_comm *comm = nullptr;
    uint64_t first = 0, last = 0;        // owned columns [first, last) of the genome
    size_t part0 = 0, part1 = 0;         // its parts [part0, part1)
    void *d_piece = nullptr;             // its piece of the statistics all-gather (kTail of epv_sampler.cpp)
    void *d_gather = nullptr;            // [slots] pieces
    void *d_halo[4] = {nullptr, nullptr, nullptr, nullptr};  // send prev, recv prev, send next, recv next
    uint64_t halo_bytes = 0;
  };
  void check(int rc, const char *what);
  void check_mcmc(int rc, const char *what);
  void check_on(epv_ctx *c, int rc, const char *what);
  void change_pattern_layouts(const std::vector<epv_ctx *> &cs, uint32_t &n_rows, uint64_t &n_samples,
                              std::vector<uint64_t> *first, std::vector<uint64_t> *count);
  void check_comm(epv_comm *c, int rc, const char *what);
  bool sharded() const { return !parts_.empty(); }
  void drop_parts();          // back to the single context ctx_
  void refresh_parts();       // equal capacities, halo columns of every inner edge, fresh halo marks
  void apply_sample_root();
  void apply_unobserved(epv_ctx *c, uint64_t lo, uint64_t hi);   // unobs_ columns [lo, hi) of the genome
  void build_fixed(uint64_t n);                                  // fixed_ of regions_ over a genome of n sites
  void apply_fixed(epv_ctx *c, uint64_t lo, uint64_t hi);        // fixed_ columns [lo, hi) of the genome
  void apply_leaf_evidence(epv_ctx *c, uint64_t lo, uint64_t hi);   // evidence_ columns [lo, hi) of the genome
  void build(const Tree &th, const FlatPaths &paths, uint64_t n_global, bool rank_mode);
  std::vector<epv_ctx *> contexts() const;
  void equalize_capacity();
  void ensure_stat_buffers();
  void free_stat_buffers();
  class Workers;              // one persistent host thread per part (epv_sampler.cpp)
  void on_parts(const std::function<void(size_t)> &f);   // f(p) for every part p, each on its part's thread; waits
  std::unique_ptr<Workers> workers_;
  epv_ctx *ctx_;              // the context of the unsharded paths (== parts_[0].ctx when sharded)
  std::vector<int> devices_;
  int contexts_wanted_ = 0;      // contexts per GPU; 0 = by tree size (3 up to 8 branches: fused colour phase; else 2)
  uint32_t row_blocks_ = 64;  // GPU slots are cut on multiples of 256 * row_blocks_ sites (EPV_ROW_BLOCKS)
  bool force_comm_ = false;   // EPV_FORCE_COMM=1: the exchange layer even for one slot (tests)
  std::vector<Part> parts_;
  std::vector<Slot> slots_;
  uint64_t halo_ = 0;         // halo columns at every inner edge (multiple of 256)
  uint64_t stat_batch_ = 0;   // batch the statistics pieces are sized for
  uint32_t capacity_;
  uint32_t pa_points_ = 0;    // set_path_average
  bool bevents_ = false;      // set_branch_events
  uint64_t wstat_W_ = 0;      // set_window_stats
  uint32_t epoch_P_ = 0;      // set_epoch_stats
  bool origins_ = false;      // set_lineage_origins
  uint64_t domains_max_ = 0; // set_domain_stats
  uint64_t turnover_max_ = 0; // set_domain_turnover
  uint64_t tracts_max_ = 0;   // set_change_tracts
  uint32_t corr_lag_ = 0;     // set_spatial_correlation
  uint64_t corr_max_ = 0;
  std::vector<uint32_t> dmaps_sizes_;   // set_domain_maps
  uint32_t dmaps_state_ = 1;
  uint64_t dmaps_max_ = 0;
  bool patterns_ = false;     // set_change_patterns
  uint32_t mixing_lag_ = 0;   // enable_mixing
  uint32_t options_ = 0;      // set_options: the word every context gets (its SAMPLE_ROOT bit follows SAMPLE_ROOT)
  std::vector<uint8_t> unobs_;   // set_unobserved: whole-genome mask of unobserved leaf cells, empty = none
  std::vector<uint64_t> regions_;   // set_regions: the lengths, empty = one region
  std::vector<uint8_t> fixed_;      // their end sites over the genome (built when the genome's length is known)
  uint64_t n_fixed_ = 0;            // the fixed sites among 1 .. n - 2: not counted in the acceptance rate
  std::vector<float> evidence_;  // set_leaf_evidence: whole-genome table of leaf evidence, empty = none
  int n_nodes_ = 0;
  uint64_t n_sites_ = 0;      // genome length (all slots)
  size_t world_ = 1;          // slots of the run (== slots_.size() unless one slot per process)
  bool rank_mode_ = false;
  RankSpec rank_;
  epv_comm *rank_comm_ = nullptr;   // one slot per process: the communicator outlives the parts
};

}  // namespace epv

#endif
