// epievo_est_params_histories -- MI355X drop-in for the reference's MCEM driver
// (/root/reference/src/prog/epievo_est_params_histories.cpp:93-300): same flags, same
// positionals, same param / Newick / local_paths formats, same per-iteration outputs and
// -v TSV line.  The E-step (reset + run_mcmc) and scale_jump_times run on the GPU; the
// O(8) M-step runs on the host.
// One extension: -g/--gpus <list> (or the environment variable EPV_DEVICES) names the GPUs of
// the node to shard the sites over -- "all", or HIP device ids "0,1,2,3" -- with RCCL between
// them (epv_sampler.hpp); results do not depend on the list.  A list with repeats ("0,0,0,0")
// rehearses a multi-GPU run on fewer GPUs.
// Another: -m/--missing STATES_FILE -- leaf cells marked N there are missing data, resampled in every
// E-step instead of pinned (SingleSiteSampler::set_unobserved; kept across the iterations).
// And: -l/--leaf-probs FILE -- P(state 1) per leaf cell in a file of the same shape (N = 0.5); cells strictly
// between 0 and 1 carry evidence in every E-step (SingleSiteSampler::set_leaf_evidence).  Not together with -m.
// And: -G/--regions FILE -- the chromosomes or gap-free stretches of the genome, `name n_sites` per line in the order
// of the paths (epv::read_regions): their end sites are held fixed in every E-step, so no update and no counted
// triple spans a break (SingleSiteSampler::set_regions; kept across the iterations).
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <limits>
#include <random>
#include <stdexcept>
#include <chrono>
#include <cmath>
#include <thread>

#include "epievo_mi355x.h"
#include "epv_io.hpp"
#include "epv_model.hpp"
#include "epv_options.hpp"
#include "epv_sampler.hpp"

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
    bool VERBOSE = false, single_branch = false, optimize_branches = false, direct_sampler = false, direct_fused = false, leaf_fast = false;
    string outfile, param_file_updated, tree_file, treefile_updated, gpu_list, missing_file, leaf_probs_file, regions_file;
    size_t iteration = 10, batch = 10, burnin = 10, paths_every = 1;
    size_t rng_seed = std::numeric_limits<size_t>::max();
    static const double param_tol = 1e-10;

    epv::OptionParser opt_parse(strip_path(argv[0]), "estimate parameters and evolutionary histories",
                                "<param> (<treefile>) <path_file>");
    opt_parse.add_opt("iteration", 'i', "number of MCMC-EM iteration", false, iteration);
    opt_parse.add_opt("batch", 'B', "number of MCMC iteration", false, batch);
    opt_parse.add_opt("burnin", 'L', "MCMC burn-in length", false, burnin);
    opt_parse.add_opt("seed", 's', "rng seed", false, rng_seed);
    opt_parse.add_opt("outfile", 'o', "output file of local paths", true, outfile);
    opt_parse.add_opt("outparam", 'p', "output file of parameters", false, param_file_updated);
    opt_parse.add_opt("outtree", 't', "output file of tree", false, treefile_updated);
    opt_parse.add_opt("single_branch", 'T', "pairwise process (assumes no tree)", false, single_branch);
    opt_parse.add_opt("branch", 'b', "optimize branch lengths", false, optimize_branches);
    opt_parse.add_opt("direct-sampler", 'j', "jump times by the direct end-conditioned sampler: bounded work per segment "
                      "whatever the rates", false, direct_sampler);
    opt_parse.add_opt("direct-fused", 'F', "the direct sampler inside the fused colour phase where that is eligible "
                      "(implies -j; same results)", false, direct_fused);
    opt_parse.add_opt("leaf-fast", 'f', "with -m / -l: keep the fused, second or large-tree proposal kernel (their leaf "
                      "variants) instead of the first (same results)", false, leaf_fast);
    opt_parse.add_opt("verbose", 'v', "print more run info", false, VERBOSE);
    opt_parse.add_opt("gpus", 'g', "GPUs to shard the sites over: all | 0,1,.. (default: EPV_DEVICES or 0)", false,
                      gpu_list);
    // extension: the reference rewrites the whole paths file after EVERY iteration (:280-283; the file
    // doubles as a checkpoint).  -e k keeps that for every k-th iteration and the last one: the final
    // file is the same bytes, the ones in between are not written
    opt_parse.add_opt("missing", 'm', "states file whose N cells are missing leaf data: resampled, not pinned", false,
                      missing_file);
    opt_parse.add_opt("leaf-probs", 'l', "file of P(state 1) per leaf cell (N = 0.5): evidence, resampled; 0 and 1 are data",
                      false, leaf_probs_file);
    opt_parse.add_opt("regions", 'G', "regions file (name n_sites per line, in the order of the paths): the first and last "
                      "site of every region are held fixed, no update and no counted triple spans a break", false,
                      regions_file);
    opt_parse.add_opt("paths-every", 'e', "write the paths file every k-th iteration and after the last (default 1: "
                      "every iteration, as the reference does)", false, paths_every);
    vector<string> leftover_args;
    opt_parse.parse(argc, argv, leftover_args);
    if (paths_every == 0) paths_every = 1;
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
    if (VERBOSE) {
      cerr << "rng seed: " << rng_seed << endl;
      cerr << "itr\tstationary\tbaseline\tinit\tacc_rate\tllh\t\n";
      cerr << "0" << "\t" << the_model.T[0] << "\t" << the_model.T[3] << "\t" << the_model.baseline[0]
           << "\t" << the_model.baseline[3] << endl;
    }

    // The reference rewrites the paths file after every iteration (:280-283).  Formatting and
    // writing 111 MB (n = 1e6, tree.nwk) takes longer than the E-step of the next iteration, and
    // that E-step needs only the device-resident paths: the file of iteration i is written by a
    // background thread while the GPU runs iteration i + 1 (same bytes, same order of files).
    std::string writer_error;
    epv::FlatPaths out_paths;
    vector<double> out_branches;
    epv::SingleSiteSampler mcmc(burnin, batch,
                                gpu_list.empty() ? epv::devices_from_env() : epv::parse_device_list(gpu_list));
    // (every context, later resets included; -f is harmless without -m / -l: the plan is then the default's)
    if (direct_sampler || direct_fused || leaf_fast)
      mcmc.set_options((direct_sampler || direct_fused ? (uint32_t)EPV_OPT_DIRECT_SAMPLER : 0u) |
                       (direct_fused ? (uint32_t)EPV_OPT_DIRECT_FUSED : 0u) | (leaf_fast ? (uint32_t)EPV_OPT_LEAF_FAST : 0u));
    if (!unobserved.empty()) mcmc.set_unobserved(std::move(unobserved));   // (applied by the first reset)
    if (!evidence.empty()) mcmc.set_leaf_evidence(std::move(evidence));
    if (!regions.empty()) mcmc.set_regions(std::move(regions));   // (kept across the iterations)
    // declared AFTER everything the thread references (and after the sampler): on an exception the
    // join runs first, while out_paths, out_branches and writer_error are still alive, and the file
    // of the last completed iteration is written out in full, as the synchronous reference leaves it
    std::thread writer;
    struct Joiner { std::thread &t; ~Joiner() { if (t.joinable()) t.join(); } } joiner{writer};
    // EPV_CLI_TIMING=1: where the wall clock of the iterations went (stderr, at the end)
    const bool timing = std::getenv("EPV_CLI_TIMING") != nullptr;
    double t_reset = 0, t_mcmc = 0, t_mstep = 0, t_scale = 0, t_wait = 0, t_download = 0;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    for (size_t itr = 0; itr < iteration; itr++) {
      double t0 = now();
      if (itr == 0) {
        mcmc.reset(the_model, th, paths);
        if (VERBOSE) cerr << "[GPU LAYOUT: " << mcmc.layout() << "]" << endl;
        if (VERBOSE && (n_held_unobserved || n_held_evidence)) {
          static const char *const kernel[] = {"first", "second", "second (segment lists)", "fused phase", "large-tree"};
          const uint32_t mode = mcmc.phase_mode();
          cerr << "[PROPOSAL KERNEL WITH " << n_held_unobserved << " UNOBSERVED AND " << n_held_evidence
               << " EVIDENCE LEAF CELLS: " << kernel[mode < 5u ? mode : 0u] << (mode ? ", leaf variant" : "") << "]" << endl;
        }
      } else {
        mcmc.reset(the_model);
      }

      t_reset += now() - t0; t0 = now();
      double acceptance_rate;
      vector<vector<double>> J_accum, D_accum;
      mcmc.run_mcmc(rng_seed, itr, J_accum, D_accum, acceptance_rate);
      t_mcmc += now() - t0; t0 = now();

      /* PARAMETER ESTIMATION (host) */
      const int B = th.n_nodes() - 1;
      vector<double> J(B * 8), D(B * 8);
      for (int b = 1; b <= B; ++b)
        for (int i = 0; i < 8; ++i) { J[(b - 1) * 8 + i] = J_accum[b][i]; D[(b - 1) * 8 + i] = D_accum[b][i]; }
      double llh = 0.0;
      if (!optimize_branches) {
        llh = epv::estimate_rates(param_tol, th.n_nodes(), J.data(), D.data(), the_model);
        epv::set_one_change_per_site_per_unit_time(the_model.rates, th.branches);
      } else {
        llh = epv::estimate_rates_and_branches(param_tol, th.n_nodes(), J.data(), D.data(), th.branches,
                                               the_model);
      }
      t_mstep += now() - t0; t0 = now();
      mcmc.scale_jump_times(th.branches);
      t_scale += now() - t0;

      if (VERBOSE)
        cerr << itr + 1 << "\t" << the_model.T[0] << "\t" << the_model.T[3] << "\t"
             << the_model.baseline[0] << "\t" << the_model.baseline[3] << "\t" << acceptance_rate
             << "\t" << llh << endl;

      if (!param_file_updated.empty()) {
        std::ofstream out_param(param_file_updated);
        // EPV_TEST_FAIL_PARAM_AT=k (tests): pretend the k-th rewrite failed, to exercise the error path
        // while the previous iteration's paths file is still being written
        const char *fail_at = std::getenv("EPV_TEST_FAIL_PARAM_AT");
        if (fail_at && (size_t)std::atol(fail_at) == itr + 1) out_param.setstate(std::ios::failbit);
        if (!out_param) throw std::runtime_error("bad output param file: " + param_file_updated);
        out_param << the_model.format_for_param_file() << endl;
      }
      if ((itr + 1) % paths_every != 0 && itr + 1 != iteration) {
        if (optimize_branches && !treefile_updated.empty()) {
          std::ofstream out_tree(treefile_updated);
          if (!out_tree) throw std::runtime_error("bad output param file: " + treefile_updated);
          out_tree << th.newick() << endl;
        }
        continue;
      }
      t0 = now();
      if (writer.joinable()) writer.join();
      if (!writer_error.empty()) throw std::runtime_error(writer_error);
      t_wait += now() - t0; t0 = now();
      mcmc.download(out_paths);
      t_download += now() - t0;
      out_branches = th.branches;
      writer = std::thread([&outfile, &th, &out_paths, &out_branches, &writer_error] {
        try {
          epv::write_local_paths(outfile, th.node_names, th.n_nodes(), out_paths.n_sites, out_branches.data(),
                                 out_paths.init.data(), out_paths.offsets.data(), out_paths.jumps.data());
        } catch (const std::exception &e) { writer_error = e.what(); }
      });
      if (optimize_branches && !treefile_updated.empty()) {
        std::ofstream out_tree(treefile_updated);
        if (!out_tree) throw std::runtime_error("bad output param file: " + treefile_updated);
        out_tree << th.newick() << endl;
      }
    }
    const double t0 = now();
    if (writer.joinable()) writer.join();
    if (!writer_error.empty()) throw std::runtime_error(writer_error);
    t_wait += now() - t0;
    if (timing)
      cerr << "[TIMING over " << iteration << " iterations, seconds: reset " << t_reset << ", run_mcmc " << t_mcmc
           << ", M-step " << t_mstep << ", scale_jump_times " << t_scale << ", waiting for the previous file "
           << t_wait << ", download " << t_download << "]" << endl;
  } catch (const std::exception &e) {
    cerr << e.what() << endl;
    return EXIT_FAILURE;
  }
  return EXIT_SUCCESS;
}
