// epievo_est_histories -- the reference's E-step program (src/prog/epievo_est_histories.cpp, which
// does not build there: SURVEY.md section 0.7) on the GPU: one run_mcmc (EM iteration 0) on the input
// paths, the final paths written in local_paths format.  Same flags as the reference
// (-B -L -s -o -T -v) plus -g as in epievo_est_params_histories; input loading and the tot_time
// rescale are that program's (epv::load_paths_and_tree).
// New: -a/--average FILE with -n/--npoints (default 100, as average_paths): the average history of
// the B batch sweeps, counted on the device (epv_set_path_average), in average_paths' output format
// (average_paths.cpp:49-63), without writing the samples to files.
// New: -m/--missing STATES_FILE: leaf cells marked N there are unobserved (SingleSiteSampler::set_unobserved):
// the MCMC resamples their end states instead of pinning them; the other cells must agree with the paths.
// New: -l/--leaf-probs FILE: a file of the same shape with P(state 1) per leaf cell (N = 0.5): cells with a
// probability strictly between 0 and 1 carry evidence (SingleSiteSampler::set_leaf_evidence) and are resampled;
// 0 and 1 are data and must agree with the paths.  Not together with -m.
// New: -G/--regions FILE: the chromosomes or gap-free stretches of the genome, `name n_sites` per line in the order of
// the paths (epv::read_regions): their end sites are held fixed, so no update and no counted triple spans a break
// (SingleSiteSampler::set_regions).  Not together with -r, -E, -d, -R, -X, -C or -D: those summaries count across
// neighbouring sites and are not cut at breaks yet, and the library refuses them by name.
// New: -c/--changes FILE with -w/--window W (default 1): the posterior branch-event maps of the B batch sweeps
// (epv_set_branch_events: end state, net gain / loss, any change, gains, losses per branch and site), summed
// over windows of W sites, as integers (epv::write_branch_events).  Changes nothing else the run writes.
// New: -r/--regional FILE with the same -w/--window W: the regional sufficient statistics of the B batch sweeps
// (epv_set_window_stats: J and D per branch and window of W sites as exact integers, then per window the sums
// over the branches and the regional rate factor under the model of the run; epv::write_window_stats).
// Changes nothing else the run writes.
// New: -O/--origins FILE with the same -w/--window W: the lineage origin maps of the B batch sweeps
// (epv_set_lineage_origins: per leaf and site on which branch of the leaf's lineage the state last changed, and
// the age of the leaf's state), summed over windows of W sites, as integers (epv::write_lineage_origins).
// Changes nothing else the run writes.
// New: -d/--domains FILE: the domain size spectra of the B batch sweeps (epv_set_domain_stats with max_samples = B:
// per node and state the spectrum of run lengths of the node's state along the genome, closed over the whole
// genome), as integers (epv::write_domain_stats).  Changes nothing else the run writes.
// New: -E/--epochs FILE with -K/--nepochs P (default 10): the epoch statistics of the B batch sweeps
// (epv_set_epoch_stats: J and D per branch and epoch of the branch as exact integers, with the epoch's rate factor
// under the model of the run; epv::write_epoch_stats).  Changes nothing else the run writes.
// New: -P/--patterns FILE with the same -w/--window W: the change patterns of the B batch sweeps
// (epv_set_change_patterns: per site what happened across the branches of the tree -- the jump spectrum, one-branch,
// parallel and reverted changes, sole gains and losses per branch, changed clades), summed over windows of W sites,
// as integers (epv::write_change_patterns).  Changes nothing else the run writes.
// New: -R/--turnover FILE: the domain turnover of the B batch sweeps (epv_set_domain_turnover with max_samples = B:
// per branch the runs of the state at its start and at its end, each kept or turned over -- domains born and died,
// gaps filled and opened -- closed over the whole genome), as integers (epv::write_domain_turnover).  Changes
// nothing else the run writes.
// New: -C/--correlation FILE with -M/--maxlag L (default 64, at most 1024): the spatial correlations of the B batch
// sweeps (epv_set_spatial_correlation with max_samples = B: per node state row and branch change row the pairs of
// ones at every lag 1 .. L, closed over the whole genome), as integers (epv::write_spatial_correlation).  Changes
// nothing else the run writes.
// New: -x/--mixing FILE with -A/--acflags K (default 8, at most 16) and the same -w/--window W: the chain mixing
// diagnostics of the B batch sweeps (epv_set_mixing: per site the linked sample pairs whose history differs, and the
// sums of the site's jump count and of its lagged products up to lag K), per window of W sites: the integer sum of
// the moves, the move rate, the pooled autocorrelations and their integrated autocorrelation time
// (epv::write_mixing).  Changes nothing else the run writes.
// New: -D/--maps FILE with -z/--sizes L1,L2,.. (default 5,20; 1 to 4 increasing sizes of 1 .. 1024), -S/--state s
// (default 1) and the same -w/--window W: the domain maps of the B batch sweeps (epv_set_domain_maps with max_samples =
// B: per node, size and site the samples in which the site lies in a run of state s of at least that size), summed
// over windows of W sites, as integers (epv::write_domain_maps).  Changes nothing else the run writes.
// New: -X/--tracts FILE: the change tracts of the B batch sweeps (epv_set_change_tracts with max_samples = B: per
// branch the maximal runs of sites with a net change, by direction (gain, loss, mixed), by the state of the unchanged
// site on each flank and by length -- domains born, grown, shrunk, split and died, and by how many sites -- closed
// over the whole genome), as integers (epv::write_change_tracts).  Changes nothing else the run writes.
#include <cstdlib>
#include <iostream>
#include <limits>
#include <random>
#include <stdexcept>

#include "epievo_mi355x.h"
#include "epv_dmaps.hpp"
#include "epv_io.hpp"
#include "epv_model.hpp"
#include "epv_options.hpp"
#include "epv_sampler.hpp"
#include "epv_tracts.hpp"

using std::cerr;
using std::endl;
using std::string;
using std::vector;

static string strip_path(const string &full) {
  const size_t p = full.find_last_of('/');
  return p == string::npos ? full : full.substr(p + 1);
}

int main(int argc, const char **argv) {
  try {
    bool VERBOSE = false, single_branch = false, direct_sampler = false, direct_fused = false, leaf_fast = false;
    string outfile, tree_file, gpu_list, regions_file, average_file, missing_file, leaf_probs_file, changes_file, regional_file, origins_file, domains_file, epochs_file, patterns_file, turnover_file, corr_file, mixing_file, maps_file, maps_sizes, tracts_file;
    size_t batch = 10, burnin = 10, n_points = 100;
    const size_t no_epochs = std::numeric_limits<size_t>::max();
    size_t n_epochs = no_epochs;
    const size_t no_lag = std::numeric_limits<size_t>::max();
    size_t max_lag = no_lag, mixing_lag = no_lag, maps_state = no_lag;
    const size_t no_window = std::numeric_limits<size_t>::max();
    size_t window = no_window;
    size_t rng_seed = std::numeric_limits<size_t>::max();

    epv::OptionParser opt_parse(strip_path(argv[0]), "estimate evolutionary histories",
                                "<param> (<treefile>) <path_file>");
    opt_parse.add_opt("batch", 'B', "number of MCMC iteration", false, batch);
    opt_parse.add_opt("burnin", 'L', "MCMC burn-in length", false, burnin);
    opt_parse.add_opt("seed", 's', "rng seed", false, rng_seed);
    opt_parse.add_opt("outfile", 'o', "output file of local paths", true, outfile);
    opt_parse.add_opt("single_branch", 'T', "pairwise process (assumes no tree)", false, single_branch);
    opt_parse.add_opt("direct-sampler", 'j', "jump times by the direct end-conditioned sampler: bounded work per segment "
                      "whatever the rates", false, direct_sampler);
    opt_parse.add_opt("direct-fused", 'F', "the direct sampler inside the fused colour phase where that is eligible "
                      "(implies -j; same results)", false, direct_fused);
    opt_parse.add_opt("leaf-fast", 'f', "with -m / -l: keep the fused, second or large-tree proposal kernel (their leaf "
                      "variants) instead of the first (same results)", false, leaf_fast);
    opt_parse.add_opt("verbose", 'v', "print more run info", false, VERBOSE);
    opt_parse.add_opt("gpus", 'g', "GPUs to shard the sites over: all | 0,1,.. (default: EPV_DEVICES or 0)", false,
                      gpu_list);
    opt_parse.add_opt("average", 'a', "output file of the average history of the batch sweeps", false, average_file);
    opt_parse.add_opt("npoints", 'n', "number of time points per branch of the average", false, n_points);
    opt_parse.add_opt("missing", 'm', "states file whose N cells are missing leaf data: resampled, not pinned", false,
                      missing_file);
    opt_parse.add_opt("regions", 'G', "regions file (name n_sites per line, in the order of the paths): the first and last "
                      "site of every region are held fixed, no update and no counted triple spans a break", false,
                      regions_file);
    opt_parse.add_opt("leaf-probs", 'l', "file of P(state 1) per leaf cell (N = 0.5): evidence, resampled; 0 and 1 are data",
                      false, leaf_probs_file);
    opt_parse.add_opt("changes", 'c', "output file of the branch-event maps of the batch sweeps (integer window sums)",
                      false, changes_file);
    opt_parse.add_opt("regional", 'r', "output file of J and D per window of the batch sweeps, with regional rate factors",
                      false, regional_file);
    opt_parse.add_opt("origins", 'O', "output file of the lineage origin maps of the batch sweeps (integer window sums)",
                      false, origins_file);
    opt_parse.add_opt("domains", 'd', "output file of the domain size spectra of the batch sweeps (integer counts per bin)",
                      false, domains_file);
    opt_parse.add_opt("epochs", 'E', "output file of J and D per branch and epoch of the batch sweeps, with rate factors",
                      false, epochs_file);
    opt_parse.add_opt("patterns", 'P', "output file of the change patterns of the batch sweeps (integer window sums)",
                      false, patterns_file);
    opt_parse.add_opt("turnover", 'R', "output file of the domain turnover of the batch sweeps (integer counts per bin)",
                      false, turnover_file);
    opt_parse.add_opt("correlation", 'C', "output file of the spatial correlations of the batch sweeps (integer pair counts "
                      "per lag)", false, corr_file);
    opt_parse.add_opt("maxlag", 'M', "largest lag of the spatial correlations (default 64, at most 1024)", false, max_lag);
    opt_parse.add_opt("mixing", 'x', "output file of the chain mixing diagnostics of the batch sweeps per window (moves, "
                      "move rate, autocorrelations of the jump count)", false, mixing_file);
    opt_parse.add_opt("acflags", 'A', "largest lag of the mixing diagnostics (default 8, at most 16)", false, mixing_lag);
    opt_parse.add_opt("maps", 'D', "output file of the domain maps of the batch sweeps (integer window sums)", false,
                      maps_file);
    opt_parse.add_opt("sizes", 'z', "sizes of the domain maps: 1 to 4 increasing numbers of sites, at most 1024 (default "
                      "5,20)", false, maps_sizes);
    opt_parse.add_opt("state", 'S', "state whose domains the maps locate: 0 or 1 (default 1)", false, maps_state);
    opt_parse.add_opt("tracts", 'X', "output file of the change tracts of the batch sweeps (integer counts per class and bin)",
                      false, tracts_file);
    opt_parse.add_opt("nepochs", 'K', "epochs per branch of the epoch statistics (default 10, at most 256)", false, n_epochs);
    opt_parse.add_opt("window", 'w', "sites per window of the branch-event maps, regional statistics, origin maps, "
                      "change patterns, mixing diagnostics and domain maps (default 1)", false, window);
    vector<string> leftover_args;
    opt_parse.parse(argc, argv, leftover_args);
    if (argc == 1 || opt_parse.help_requested()) {
      cerr << opt_parse.help_message() << endl << opt_parse.about_message() << endl;
      return EXIT_SUCCESS;
    }
    if (opt_parse.option_missing()) {
      cerr << opt_parse.option_missing_message() << endl;
      return EXIT_SUCCESS;
    }
    if (leftover_args.size() == 2) {
      if (!single_branch) { cerr << opt_parse.help_message() << endl; return EXIT_SUCCESS; }
    } else if (leftover_args.size() != 3) {
      cerr << opt_parse.help_message() << endl;
      return EXIT_SUCCESS;
    } else {
      tree_file = leftover_args[1];
    }
    if (!average_file.empty() && (n_points < 2 || n_points > 0xffffffffu))
      throw std::runtime_error("-n: the number of points must be at least 2");
    if (window != no_window && changes_file.empty() && regional_file.empty() && origins_file.empty() &&
        patterns_file.empty() && mixing_file.empty() && maps_file.empty())
      throw std::runtime_error("-w/--window belongs to -c/--changes, -r/--regional, -O/--origins, -P/--patterns, "
                               "-x/--mixing and -D/--maps: give the output file of the branch-event maps, of the "
                               "regional statistics, of the origin maps, of the change patterns, of the mixing "
                               "diagnostics or of the domain maps");
    if (n_epochs != no_epochs && epochs_file.empty())
      throw std::runtime_error("-K/--nepochs belongs to -E/--epochs: give the output file of the epoch statistics");
    if (n_epochs == no_epochs) n_epochs = 10;
    if (n_epochs == 0 || n_epochs > EPV_EPOCH_MAX_P) throw std::runtime_error("-K: 1 to 256 epochs per branch");
    if (max_lag != no_lag && corr_file.empty())
      throw std::runtime_error("-M/--maxlag belongs to -C/--correlation: give the output file of the spatial correlations");
    if (max_lag == no_lag) max_lag = 64;
    if (max_lag == 0 || max_lag > 1024) throw std::runtime_error("-M: a largest lag of 1 to 1024 sites");
    if (mixing_lag != no_lag && mixing_file.empty())
      throw std::runtime_error("-A/--acflags belongs to -x/--mixing: give the output file of the mixing diagnostics");
    if (mixing_lag == no_lag) mixing_lag = 8;
    if (mixing_lag == 0 || mixing_lag > 16) throw std::runtime_error("-A: a largest lag of 1 to 16 samples");
    if ((!maps_sizes.empty() || maps_state != no_lag) && maps_file.empty())
      throw std::runtime_error("-z/--sizes and -S/--state belong to -D/--maps: give the output file of the domain maps");
    if (maps_state == no_lag) maps_state = 1;
    if (maps_state > 1) throw std::runtime_error("-S: the state is 0 or 1");
    vector<uint32_t> map_sizes;
    if (!maps_file.empty()) {
      const string text = maps_sizes.empty() ? "5,20" : maps_sizes;
      for (size_t a = 0; a <= text.size();) {
        const size_t b = std::min(text.find(',', a), text.size());
        const string item = text.substr(a, b - a);
        if (item.empty() || item.size() > 4 || item.find_first_not_of("0123456789") != string::npos)
          throw std::runtime_error("-z: sizes are numbers of sites separated by commas, as in 5,20");
        map_sizes.push_back((uint32_t)std::stoul(item));
        a = b + 1;
      }
      epv::check_domain_map_sizes((uint32_t)map_sizes.size(), map_sizes.data(), "-z");
      if (batch > (1ull << 21)) throw std::runtime_error("-D/--maps: the domain maps take at most 2^21 batch sweeps (-B)");
    }
    if (window == 0) throw std::runtime_error("-w: a window holds at least one site");
    if (window == no_window) window = 1;
    if (batch == 0) throw std::runtime_error("-B: at least one batch sweep");
    if (!turnover_file.empty() && batch > (1ull << 21))
      throw std::runtime_error("-R/--turnover: the domain turnover takes at most 2^21 batch sweeps (-B)");
    if (!tracts_file.empty() && batch > (1ull << 21))
      throw std::runtime_error("-X/--tracts: the change tracts take at most 2^21 batch sweeps (-B)");
    if (!corr_file.empty() && batch > (1ull << 21))
      throw std::runtime_error("-C/--correlation: the spatial correlations take at most 2^21 batch sweeps (-B)");
    const string param_file(leftover_args.front()), input_file(leftover_args.back());

    if (VERBOSE) cerr << "[READING PARAMETERS: " << param_file << "]" << endl;
    epv::Model the_model = epv::Model::read(param_file);
    the_model.scale_triplet_rates();
    vector<string> node_names;
    epv::FlatPaths paths;
    epv::Tree th;
    epv::load_paths_and_tree(input_file, tree_file, single_branch, VERBOSE, paths, node_names, th);
    if (!missing_file.empty() && !leaf_probs_file.empty())
      throw std::runtime_error("-m/--missing and -l/--leaf-probs cannot be given together (N in a -l file is a missing cell)");
    // missing leaf data, checked against the paths before any GPU call
    uint64_t n_held_unobserved = 0, n_held_evidence = 0;   // (for -v: beside the proposal kernel the plan takes)
    vector<uint8_t> unobserved;
    if (!missing_file.empty()) {
      uint64_t n_unobserved = 0, n_leaf_cells = 0;
      unobserved = epv::unobserved_leaf_cells(missing_file, th, paths, n_unobserved, n_leaf_cells);
      if (VERBOSE) cerr << "[UNOBSERVED LEAF CELLS: " << n_unobserved << " of " << n_leaf_cells << "]" << endl;
      n_held_unobserved = n_unobserved;
    }
    // genomic regions, likewise
    vector<uint64_t> regions;
    if (!regions_file.empty()) {
      regions = epv::read_regions(regions_file, paths.n_sites);
      if (VERBOSE) cerr << "[REGIONS: " << regions.size() << " OVER " << paths.n_sites << " SITES]" << endl;
    }
    // leaf evidence, likewise
    vector<float> evidence;
    if (!leaf_probs_file.empty()) {
      uint64_t n_evidence = 0, n_leaf_cells = 0;
      evidence = epv::leaf_evidence_cells(leaf_probs_file, th, paths, n_evidence, n_leaf_cells);
      if (VERBOSE) cerr << "[LEAF CELLS WITH EVIDENCE: " << n_evidence << " of " << n_leaf_cells << "]" << endl;
      n_held_evidence = n_evidence;
    }

    if (rng_seed == std::numeric_limits<size_t>::max()) {
      std::random_device rd;
      rng_seed = rd();
    }
    if (VERBOSE) cerr << "rng seed: " << rng_seed << endl;

    epv::SingleSiteSampler mcmc(burnin, batch,
                                gpu_list.empty() ? epv::devices_from_env() : epv::parse_device_list(gpu_list));
    // (every context, later resets included; -f is harmless without -m / -l: the plan is then the default's)
    if (direct_sampler || direct_fused || leaf_fast)
      mcmc.set_options((direct_sampler || direct_fused ? (uint32_t)EPV_OPT_DIRECT_SAMPLER : 0u) |
                       (direct_fused ? (uint32_t)EPV_OPT_DIRECT_FUSED : 0u) | (leaf_fast ? (uint32_t)EPV_OPT_LEAF_FAST : 0u));
    if (!unobserved.empty()) mcmc.set_unobserved(std::move(unobserved));   // (applied by the first reset)
    if (!evidence.empty()) mcmc.set_leaf_evidence(std::move(evidence));
    if (!regions.empty()) mcmc.set_regions(std::move(regions));
    mcmc.reset(the_model, th, paths);
    if (VERBOSE) cerr << "[GPU LAYOUT: " << mcmc.layout() << "]" << endl;
    if (VERBOSE && (n_held_unobserved || n_held_evidence)) {
      static const char *const kernel[] = {"first", "second", "second (segment lists)", "fused phase", "large-tree"};
      const uint32_t mode = mcmc.phase_mode();
      cerr << "[PROPOSAL KERNEL WITH " << n_held_unobserved << " UNOBSERVED AND " << n_held_evidence
           << " EVIDENCE LEAF CELLS: " << kernel[mode < 5u ? mode : 0u] << (mode ? ", leaf variant" : "") << "]" << endl;
    }
    if (!average_file.empty()) mcmc.set_path_average((uint32_t)n_points);
    if (!changes_file.empty()) mcmc.set_branch_events(true);
    if (!regional_file.empty()) mcmc.set_window_stats(window);
    if (!origins_file.empty()) mcmc.set_lineage_origins(true);
    if (!domains_file.empty()) mcmc.set_domain_stats(batch);
    if (!epochs_file.empty()) mcmc.set_epoch_stats((uint32_t)n_epochs);
    if (!patterns_file.empty()) mcmc.set_change_patterns(true);
    if (!turnover_file.empty()) mcmc.set_domain_turnover(batch);
    if (!corr_file.empty()) mcmc.set_spatial_correlation((uint32_t)max_lag, batch);
    if (!mixing_file.empty()) mcmc.enable_mixing((uint32_t)mixing_lag);
    if (!maps_file.empty()) mcmc.set_domain_maps(map_sizes, (uint32_t)maps_state, batch);
    if (!tracts_file.empty()) mcmc.set_change_tracts(batch);
    double acceptance_rate = 0.0;
    vector<vector<double>> J, D;
    mcmc.run_mcmc(rng_seed, 0, J, D, acceptance_rate);
    if (VERBOSE) cerr << "[ACCEPTANCE RATE: " << acceptance_rate << "]" << endl;

    epv::FlatPaths out;
    mcmc.download(out);
    if (VERBOSE) cerr << "[WRITING PATHS: " << outfile << "]" << endl;
    epv::write_local_paths(outfile, th.node_names, th.n_nodes(), out.n_sites, th.branches.data(), out.init.data(),
                           out.offsets.data(), out.jumps.data());
    if (!average_file.empty()) {
      vector<uint32_t> counts;
      uint64_t n_samples = 0;
      mcmc.download_path_average(counts, n_samples);
      if (VERBOSE) cerr << "[WRITING AVERAGE OF " << n_samples << " SAMPLES: " << average_file << "]" << endl;
      epv::write_path_average(average_file, th.node_names, th.n_nodes(), out.n_sites, (uint32_t)n_points,
                              th.branches.data(), counts.data(), n_samples);
    }
    if (!changes_file.empty()) {
      vector<uint64_t> sums;
      uint64_t n_samples = 0;
      mcmc.download_branch_event_windows(window, sums, n_samples);
      if (VERBOSE) cerr << "[WRITING BRANCH EVENTS OF " << n_samples << " SAMPLES: " << changes_file << "]" << endl;
      epv::write_branch_events(changes_file, th.node_names, th.n_nodes(), mcmc.branch_event_windows(window), window,
                               th.branches.data(), sums.data(), n_samples);
    }
    if (!regional_file.empty()) {
      vector<int64_t> counts;
      vector<double> Jw, Dw;
      uint64_t n_samples = 0, W = 0, n_windows = 0;
      mcmc.download_window_stats(counts, W, n_windows, n_samples);
      mcmc.window_counts_to_stats(counts, n_windows, n_samples, Jw, Dw);
      const vector<int> scale_exp = mcmc.window_stats_scale_exps();   // the accumulator's own k_b
      if (VERBOSE) cerr << "[WRITING REGIONAL STATISTICS OF " << n_samples << " SAMPLES: " << regional_file << "]" << endl;
      epv::write_window_stats(regional_file, th.node_names, th.n_nodes(), n_windows, W, th.branches.data(),
                              scale_exp.data(), counts.data(), n_samples, Jw.data(), Dw.data(), the_model.rates);
    }
    if (!origins_file.empty()) {
      vector<uint32_t> leaf_node, branch_node;
      vector<uint64_t> origin, age;
      uint64_t n_samples = 0;
      int k = 0;
      mcmc.lineage_origin_rows(leaf_node, branch_node);
      mcmc.download_lineage_origin_windows(window, origin, age, k, n_samples);
      if (VERBOSE) cerr << "[WRITING LINEAGE ORIGINS OF " << n_samples << " SAMPLES: " << origins_file << "]" << endl;
      epv::write_lineage_origins(origins_file, th.node_names, leaf_node.size(), leaf_node.data(), branch_node.data(),
                                 mcmc.branch_event_windows(window), window, k, origin.data(), age.data(), n_samples);
    }
    if (!domains_file.empty()) {
      vector<uint64_t> hist, len_sum;
      uint32_t n_nodes = 0;
      uint64_t n_samples = 0;
      mcmc.download_domain_stats(hist, len_sum, n_nodes, n_samples);
      if (VERBOSE) cerr << "[WRITING DOMAIN SIZE SPECTRA OF " << n_samples << " SAMPLES: " << domains_file << "]" << endl;
      epv::write_domain_stats(domains_file, th.node_names, n_samples, hist.data(), len_sum.data());
    }
    if (!epochs_file.empty()) {
      vector<uint64_t> closed, fixT;
      vector<int> scale_exp;
      uint64_t n_samples = 0;
      mcmc.download_epoch_stats(closed, scale_exp, fixT, n_samples);
      if (VERBOSE) cerr << "[WRITING EPOCH STATISTICS OF " << n_samples << " SAMPLES: " << epochs_file << "]" << endl;
      epv::write_epoch_stats(epochs_file, th.node_names, th.n_nodes(), (uint32_t)n_epochs, th.branches.data(),
                             scale_exp.data(), fixT.data(), closed.data(), n_samples, the_model.rates);
    }
    if (!patterns_file.empty()) {
      vector<uint64_t> sums;
      uint32_t n_rows = 0;
      uint64_t n_samples = 0;
      mcmc.download_change_pattern_windows(window, sums, n_rows, n_samples);
      if (VERBOSE) cerr << "[WRITING CHANGE PATTERNS OF " << n_samples << " SAMPLES: " << patterns_file << "]" << endl;
      epv::write_change_patterns(patterns_file, th.node_names, th.subtree_sizes, n_rows, out.n_sites,
                                 mcmc.branch_event_windows(window), window, sums.data(), n_samples);
    }
    if (!turnover_file.empty()) {
      vector<uint64_t> hist, len_sum;
      uint32_t n_rows = 0;
      uint64_t n_samples = 0;
      mcmc.download_domain_turnover(hist, len_sum, n_rows, n_samples);
      if (VERBOSE) cerr << "[WRITING DOMAIN TURNOVER OF " << n_samples << " SAMPLES: " << turnover_file << "]" << endl;
      const vector<string> branch_names(th.node_names.begin() + 1, th.node_names.end());
      epv::write_domain_turnover(turnover_file, branch_names, n_samples, hist.data(), len_sum.data());
    }
    if (!corr_file.empty()) {
      vector<uint64_t> n11, left1, right1;
      uint32_t n_rows = 0, L = 0;
      uint64_t n_samples = 0;
      mcmc.download_spatial_correlation(n11, left1, right1, n_rows, L, n_samples);
      if (VERBOSE) cerr << "[WRITING SPATIAL CORRELATIONS OF " << n_samples << " SAMPLES: " << corr_file << "]" << endl;
      epv::write_spatial_correlation(corr_file, th.node_names, n_samples, out.n_sites, L, n11.data(), left1.data(),
                                     right1.data());
    }
    if (!mixing_file.empty()) {
      vector<uint64_t> words, sums;
      vector<uint32_t> moved;
      mcmc.download_mixing(words, moved, sums);
      if (VERBOSE) cerr << "[WRITING MIXING DIAGNOSTICS OF " << words[0] << " SAMPLES: " << mixing_file << "]" << endl;
      epv::write_mixing(mixing_file, (uint32_t)mixing_lag, words.data(), moved.size(), window, moved.data(), sums.data());
    }
    if (!maps_file.empty()) {
      vector<uint32_t> counts;
      vector<uint64_t> edges;
      uint32_t n_nodes = 0;
      uint64_t n_samples = 0, n_sites = 0;
      mcmc.download_domain_maps(counts, edges, n_nodes, n_samples, n_sites);
      if (VERBOSE) cerr << "[WRITING DOMAIN MAPS OF " << n_samples << " SAMPLES: " << maps_file << "]" << endl;
      vector<uint64_t> sums((size_t)n_nodes * map_sizes.size() * ((n_sites + window - 1u) / window), 0u);
      epv::domain_map_windows(n_nodes, (uint32_t)map_sizes.size(), n_sites, counts.data(), window, sums.data());
      epv::write_domain_maps(maps_file, th.node_names, n_samples, (uint32_t)maps_state, map_sizes, n_sites, window,
                             sums.data());
    }
    if (!tracts_file.empty()) {
      vector<uint64_t> hist, len_sum;
      uint32_t n_branches = 0;
      uint64_t n_samples = 0;
      mcmc.download_change_tracts(hist, len_sum, n_branches, n_samples);
      if (VERBOSE) cerr << "[WRITING CHANGE TRACTS OF " << n_samples << " SAMPLES: " << tracts_file << "]" << endl;
      const vector<string> branch_names(th.node_names.begin() + 1, th.node_names.end());
      epv::write_change_tracts(tracts_file, branch_names, n_samples, hist.data(), len_sum.data());
    }
  } catch (const std::exception &e) {
    cerr << e.what() << endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
