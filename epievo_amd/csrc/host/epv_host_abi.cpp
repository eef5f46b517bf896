// epv_host_abi.cpp -- flat C face of the host-side library (libepv_host.so) so that
// Python tests / bench.py can drive the same C++ host code the CLI programs use.
// No GPU code here; no exceptions cross the boundary (non-zero return = failure,
// message via epvh_last_error).
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "epv_model.hpp"
#include "epv_sim.hpp"
#include "epv_io.hpp"
#include "epv_domains.hpp"
#include "epv_turnover.hpp"
#include "epv_tracts.hpp"
#include "epv_corr.hpp"
#include "epv_dmaps.hpp"
#include "epv_epochs.hpp"
#include "epv_indep.hpp"
#include "epv_forward.hpp"
#include "epievo_mi355x.h"
#include "../epv_plan.h"

namespace {
thread_local std::string g_err;
void put_model(const epv::Model &m, double *rates, double *T, double *baseline) {
  for (int i = 0; i < 8; ++i) rates[i] = m.rates[i];
  for (int i = 0; i < 4; ++i) { T[i] = m.T[i]; baseline[i] = m.baseline[i]; }
}
void put_text(const std::string &s, char *buf, int len) {
  if (!buf || len <= 0) return;
  std::strncpy(buf, s.c_str(), (size_t)len - 1);
  buf[len - 1] = '\0';
}
}  // namespace

#define EPVH_API extern "C" __attribute__((visibility("default")))

EPVH_API const char *epvh_last_error() { return g_err.c_str(); }

// read_model (+ optional scale_triplet_rates), est_params_histories.cpp:169-171
EPVH_API int epvh_model_read(const char *param_file, int scale, double *rates, double *T,
                             double *baseline) {
  try {
    epv::Model m = epv::Model::read(param_file);
    if (scale) m.scale_triplet_rates();
    put_model(m, rates, T, baseline);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}

EPVH_API double epvh_rate_scaling_factor(const double *rates) {
  std::array<double, 8> r;
  for (int i = 0; i < 8; ++i) r[i] = rates[i];
  return epv::rate_scaling_factor(r);
}

// the M-step exactly as the EM driver sequences it (est_params_histories.cpp:253-263).
// rates/branches are in-out; T, baseline, param_text are outputs; returns 0 / non-zero.
EPVH_API int epvh_m_step(int optimize_branches, int n_nodes, const double *J, const double *D,
                         double *rates, double *T, double *baseline, double *branches,
                         double *llh, char *param_text, int param_text_len) {
  try {
    epv::Model m;
    std::array<double, 8> r;
    for (int i = 0; i < 8; ++i) r[i] = rates[i];
    m.rebuild_from_triplet_rates(r);
    std::vector<double> br(branches, branches + n_nodes);
    if (!optimize_branches) {
      *llh = epv::estimate_rates(1e-10, n_nodes, J, D, m);
      epv::set_one_change_per_site_per_unit_time(m.rates, br);
    } else {
      *llh = epv::estimate_rates_and_branches(1e-10, n_nodes, J, D, br, m);
    }
    put_model(m, rates, T, baseline);
    for (int b = 0; b < n_nodes; ++b) branches[b] = br[b];
    put_text(m.format_for_param_file(), param_text, param_text_len);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}

// ---- forward simulation of synthetic histories
EPVH_API void *epvh_simulate(const double *rates, const double *T, int n_nodes,
                             const uint32_t *parent, const double *branches,
                             uint64_t n_sites, uint64_t seed) {
  try {
    epv::Model m;
    for (int i = 0; i < 8; ++i) m.rates[i] = rates[i];
    for (int i = 0; i < 4; ++i) m.T[i] = T[i];
    epv::FlatPaths *fp = new epv::FlatPaths(
        epv::simulate_histories(m, n_nodes, parent, branches, n_sites, seed));
    return fp;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
EPVH_API uint64_t epvh_paths_total_jumps(void *h) {
  return static_cast<epv::FlatPaths *>(h)->jumps.size();
}
EPVH_API uint64_t epvh_paths_n_sites(void *h) { return static_cast<epv::FlatPaths *>(h)->n_sites; }
EPVH_API int epvh_paths_n_nodes(void *h) { return static_cast<epv::FlatPaths *>(h)->n_nodes; }
EPVH_API void epvh_paths_copy(void *h, uint8_t *init, uint64_t *offsets, double *jumps) {
  const epv::FlatPaths *fp = static_cast<epv::FlatPaths *>(h);
  std::memcpy(init, fp->init.data(), fp->init.size());
  std::memcpy(offsets, fp->offsets.data(), fp->offsets.size() * sizeof(uint64_t));
  if (!fp->jumps.empty())
    std::memcpy(jumps, fp->jumps.data(), fp->jumps.size() * sizeof(double));
}
EPVH_API void epvh_paths_free(void *h) { delete static_cast<epv::FlatPaths *>(h); }

// ---- file formats (local_paths, Newick tree)
EPVH_API void *epvh_read_paths(const char *path_file, char *names_buf, int names_len,
                               double *tot_times, int max_nodes) {
  try {
    std::vector<std::string> names;
    std::vector<double> tt;
    epv::FlatPaths *fp = new epv::FlatPaths(epv::read_local_paths(path_file, names, tt));
    std::string joined;
    for (size_t i = 0; i < names.size(); ++i) joined += (i ? "\n" : "") + names[i];
    put_text(joined, names_buf, names_len);
    for (int b = 0; b < fp->n_nodes && b < max_nodes; ++b) tot_times[b] = tt[b];
    return fp;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}

EPVH_API int epvh_write_paths(const char *path_file, const char *names_joined, int n_nodes,
                              uint64_t n_sites, const double *tot_times, const uint8_t *init,
                              const uint64_t *offsets, const double *jumps) {
  try {
    std::vector<std::string> names;
    std::string cur;
    for (const char *p = names_joined;; ++p) {
      if (*p == '\n' || *p == '\0') { names.push_back(cur); cur.clear(); if (!*p) break; }
      else cur.push_back(*p);
    }
    epv::write_local_paths(path_file, names, n_nodes, n_sites, tot_times, init, offsets, jumps);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}

// parse a Newick file into pre-order arrays; returns n_nodes (<= max_nodes) or -1
EPVH_API int epvh_read_tree(const char *tree_file, int max_nodes, uint32_t *subtree,
                            uint32_t *parent, double *branches, char *names_buf,
                            int names_len) {
  try {
    epv::Tree t = epv::Tree::read(tree_file);
    const int n = (int)t.subtree_sizes.size();
    if (n > max_nodes) { g_err = "tree too large"; return -1; }
    std::string joined;
    for (int i = 0; i < n; ++i) {
      subtree[i] = t.subtree_sizes[i];
      parent[i] = t.parent_ids[i];
      branches[i] = t.branches[i];
      joined += (i ? "\n" : "") + t.node_names[i];
    }
    put_text(joined, names_buf, names_len);
    return n;
  } catch (const std::exception &e) { g_err = e.what(); return -1; }
}

// the tree of a Newick file printed back (Tree::newick) -- the -t output of the drop-in CLIs
EPVH_API int epvh_tree_newick(const char *tree_file, char *out, int out_len) {
  try {
    put_text(epv::Tree::read(tree_file).newick(), out, out_len);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}

// ---- global_jumps and states files (epievo_sim's outputs)
namespace {
std::vector<std::string> split_lines(const char *joined) {
  std::vector<std::string> names;
  std::string cur;
  for (const char *p = joined;; ++p) {
    if (*p == '\n' || *p == '\0') { names.push_back(cur); cur.clear(); if (!*p) break; }
    else cur.push_back(*p);
  }
  return names;
}
struct GlobalFile { std::vector<uint8_t> root; std::vector<std::string> names; std::vector<std::vector<epv::GlobalJump>> paths; };
struct StatesFile { std::vector<std::string> names; std::vector<std::vector<uint8_t>> states; };
}  // namespace

EPVH_API int epvh_write_global_jumps(const char *file, int n_nodes, const char *names_joined, uint64_t n_sites,
                                     const uint8_t *root, const uint64_t *node_offsets, const double *times,
                                     const uint64_t *positions) {
  try {
    std::vector<std::vector<epv::GlobalJump>> paths(n_nodes);
    for (int b = 1; b < n_nodes; ++b)
      for (uint64_t i = node_offsets[b]; i < node_offsets[b + 1]; ++i) paths[b].push_back({times[i], (size_t)positions[i]});
    epv::write_global_jumps(file, split_lines(names_joined), std::vector<uint8_t>(root, root + n_sites), paths);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_global_jumps(const char *file, int *n_nodes, uint64_t *n_sites, uint64_t *total) {
  try {
    GlobalFile *g = new GlobalFile();
    epv::read_global_jumps(file, g->root, g->names, g->paths);
    *n_nodes = (int)g->paths.size();
    *n_sites = g->root.size();
    uint64_t tot = 0;
    for (const auto &v : g->paths) tot += v.size();
    *total = tot;
    return g;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
EPVH_API void epvh_global_jumps_copy(void *h, uint8_t *root, uint64_t *node_offsets, double *times,
                                     uint64_t *positions, char *names, int names_len) {
  GlobalFile *g = static_cast<GlobalFile *>(h);
  std::memcpy(root, g->root.data(), g->root.size());
  uint64_t at = 0;
  for (size_t b = 0; b < g->paths.size(); ++b) {
    node_offsets[b] = at;
    for (const epv::GlobalJump &j : g->paths[b]) { times[at] = j.timepoint; positions[at] = j.position; ++at; }
  }
  node_offsets[g->paths.size()] = at;
  std::string joined;
  for (size_t i = 0; i < g->names.size(); ++i) joined += (i ? "\n" : "") + g->names[i];
  put_text(joined, names, names_len);
  delete g;
}

// states[seq][site] row-major; `names_joined` = the column names of the header line
EPVH_API int epvh_write_states(const char *file, int only_leaves, int n_nodes, const uint32_t *subtree,
                               const char *names_joined, uint64_t n_sites, const uint8_t *states) {
  try {
    epv::Tree t;
    t.subtree_sizes.assign(subtree, subtree + n_nodes);
    t.parent_ids.assign(n_nodes, 0);
    t.branches.assign(n_nodes, 0.0);
    t.node_names = split_lines(names_joined);
    std::vector<std::vector<uint8_t>> seqs(n_nodes);
    for (int b = 0; b < n_nodes; ++b) seqs[b].assign(states + (uint64_t)b * n_sites, states + (uint64_t)(b + 1) * n_sites);
    epv::write_states(file, only_leaves != 0, t, seqs);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_states(const char *file, int *n_seqs, uint64_t *n_sites) {
  try {
    StatesFile *f = new StatesFile();
    epv::read_states_file(file, f->names, f->states);
    *n_seqs = (int)f->states.size();
    *n_sites = f->states.empty() ? 0 : f->states[0].size();
    return f;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
EPVH_API void epvh_states_copy(void *h, uint8_t *states, char *names, int names_len) {
  StatesFile *f = static_cast<StatesFile *>(h);
  uint64_t at = 0;
  for (const auto &sq : f->states) { std::memcpy(states + at, sq.data(), sq.size()); at += sq.size(); }
  std::string joined;
  for (size_t i = 0; i < f->names.size(); ++i) joined += (i ? "\n" : "") + f->names[i];
  put_text(joined, names, names_len);
  delete f;
}

// ---- site-independent stage of epievo_initialization (host parts)
EPVH_API int epvh_indep_m_step(int optimize_branches, int n_nodes, const double *J, const double *D,
                               double *rates, double *branches) {
  try {
    if (!optimize_branches) {
      epv::estimate_rates_indep(n_nodes, J, D, rates);
    } else {
      std::vector<double> br(branches, branches + n_nodes);
      epv::estimate_rates_and_branches_indep(n_nodes, J, D, rates, br);
      for (int b = 0; b < n_nodes; ++b) branches[b] = br[b];
    }
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}

EPVH_API int epvh_model_from_indep_rates(const double *rates2, double *rates, double *T, double *baseline) {
  try {
    put_model(epv::model_from_indep_rates(rates2), rates, T, baseline);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}

// states: [n_nodes][n_sites] row-major, updated in place with the drawn internal states
EPVH_API void *epvh_initialize_paths_heuristic(uint64_t seed, int n_nodes, const uint32_t *subtree,
                                               const uint32_t *parent, const double *branches,
                                               uint64_t n_sites, uint8_t *states) {
  try {
    epv::Tree t;
    t.subtree_sizes.assign(subtree, subtree + n_nodes);
    t.parent_ids.assign(parent, parent + n_nodes);
    t.branches.assign(branches, branches + n_nodes);
    t.node_names.assign(n_nodes, "");
    std::vector<std::vector<uint8_t>> st(n_nodes);
    for (int b = 0; b < n_nodes; ++b) st[b].assign(states + (uint64_t)b * n_sites, states + (uint64_t)(b + 1) * n_sites);
    epv::FlatPaths *fp = new epv::FlatPaths(epv::initialize_paths_heuristic(seed, t, st));
    for (int b = 0; b < n_nodes; ++b) std::memcpy(states + (uint64_t)b * n_sites, st[b].data(), n_sites);
    return fp;
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}

// ---- forward simulation (epievo_sim): same outputs as the test shim's ref_forward_sim
EPVH_API uint64_t epvh_forward_sim(uint64_t seed, const double *rates, const double *T, int n_nodes,
                                   const uint32_t *parent, const double *branches, uint64_t n_sites,
                                   uint8_t *sequences, uint64_t *jump_offsets, double *jump_times,
                                   uint64_t *jump_positions, uint64_t cap) {
  epv::Model m;
  for (int i = 0; i < 8; ++i) m.rates[i] = rates[i];
  for (int i = 0; i < 4; ++i) m.T[i] = T[i];
  epv::Tree th;
  th.parent_ids.assign(parent, parent + n_nodes);
  th.branches.assign(branches, branches + n_nodes);
  th.subtree_sizes.assign(n_nodes, 1);   // only n_nodes() is needed here
  th.node_names.assign(n_nodes, "");
  std::mt19937 gen(seed);
  std::vector<uint8_t> root;
  epv::sample_root(m, n_sites, gen, root);
  std::vector<std::vector<uint8_t>> seqs;
  std::vector<std::vector<epv::GlobalJump>> paths;
  std::vector<size_t> events;
  epv::simulate_tree(m, th, root, gen, seqs, paths, events);
  uint64_t tot = 0;
  jump_offsets[0] = 0;
  for (int node = 0; node < n_nodes; ++node) {
    for (const epv::GlobalJump &j : paths[node]) {
      if (tot < cap) { jump_times[tot] = j.timepoint; jump_positions[tot] = j.position; }
      ++tot;
    }
    jump_offsets[node + 1] = tot;
    std::memcpy(sequences + (uint64_t)node * n_sites, seqs[node].data(), n_sites);
  }
  return tot;
}

// ---- regional sufficient statistics: the rate factor per window, and the file of epievo_est_histories -r
// J, D: [n_windows][n_nodes-1][8]; out[n_windows] (NaN for a window without dwell time)
EPVH_API void epvh_regional_rate_factors(int n_nodes, uint64_t n_windows, const double *J, const double *D,
                                         const double *rates, double *out) {
  std::array<double, 8> r;
  for (int i = 0; i < 8; ++i) r[i] = rates[i];
  const uint64_t step = (uint64_t)(n_nodes - 1) * 8u;
  for (uint64_t w = 0; w < n_windows; ++w) out[w] = epv::regional_rate_factor(n_nodes, J + w * step, D + w * step, r);
}
EPVH_API double epvh_collapsed_log_likelihood(int n_nodes, const double *J, const double *D, const double *rates) {
  std::array<double, 8> r;
  for (int i = 0; i < 8; ++i) r[i] = rates[i];
  return epv::collapsed_log_likelihood(n_nodes, J, D, r);
}
// node_names: n_nodes names joined by '\n' (the root's first); branch_len, scale_exp: [n_nodes], index 0 = root
EPVH_API int epvh_write_window_stats(const char *file, const char *node_names, int n_nodes, uint64_t n_windows,
                                     uint64_t window, const double *branch_len, const int *scale_exp,
                                     const int64_t *counts, uint64_t n_samples, const double *J, const double *D,
                                     const double *rates) {
  try {
    std::vector<std::string> names;
    std::string all(node_names), cur;
    for (char ch : all) {
      if (ch == '\n') { names.push_back(cur); cur.clear(); } else cur.push_back(ch);
    }
    names.push_back(cur);
    if ((int)names.size() != n_nodes) throw std::runtime_error("epvh_write_window_stats: one name per node");
    std::array<double, 8> r;
    for (int i = 0; i < 8; ++i) r[i] = rates[i];
    epv::write_window_stats(file, names, n_nodes, n_windows, window, branch_len, scale_exp, counts, n_samples, J, D, r);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_window_stats(const char *file) {
  try {
    return new epv::WindowStats(epv::read_window_stats(file));
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
static std::string joined_names(const epv::WindowStats *ws) {
  std::string joined;
  for (size_t i = 0; i < ws->node_names.size(); ++i) joined += (i ? "\n" : "") + ws->node_names[i];
  return joined;
}
// names_len: the bytes epvh_window_stats_copy needs for the names, the closing 0 included
EPVH_API void epvh_window_stats_dims(void *h, uint64_t *n_samples, uint64_t *window, uint64_t *n_windows,
                                     uint64_t *n_branches, uint64_t *names_len) {
  const epv::WindowStats *ws = (const epv::WindowStats *)h;
  *names_len = joined_names(ws).size() + 1u;
  *n_samples = ws->n_samples;
  *window = ws->window;
  *n_windows = ws->n_windows;
  *n_branches = ws->node_names.size();
}
// names: the non-root nodes' names joined by '\n'; branch_len, scale_exp: [B]; counts [nw][B][16]; all_J, all_D
// [nw][8]; factor [nw]
EPVH_API void epvh_window_stats_copy(void *h, char *names, int names_len, double *branch_len, int *scale_exp,
                                     int64_t *counts, int64_t *all_J, double *all_D, double *factor) {
  const epv::WindowStats *ws = (const epv::WindowStats *)h;
  put_text(joined_names(ws), names, names_len);
  std::copy(ws->branch_len.begin(), ws->branch_len.end(), branch_len);
  std::copy(ws->scale_exp.begin(), ws->scale_exp.end(), scale_exp);
  std::copy(ws->counts.begin(), ws->counts.end(), counts);
  std::copy(ws->all_J.begin(), ws->all_J.end(), all_J);
  std::copy(ws->all_D.begin(), ws->all_D.end(), all_D);
  std::copy(ws->factor.begin(), ws->factor.end(), factor);
}
EPVH_API void epvh_window_stats_free(void *h) { delete (epv::WindowStats *)h; }

// ---- lineage origin maps: the file of epievo_est_histories -O
static std::vector<std::string> split_names(const char *joined) {
  std::vector<std::string> names;
  std::string cur;
  for (const char *p = joined; *p; ++p) {
    if (*p == '\n') { names.push_back(cur); cur.clear(); } else cur.push_back(*p);
  }
  names.push_back(cur);
  return names;
}
static std::string join_names(const std::vector<std::string> &names) {
  std::string joined;
  for (size_t i = 0; i < names.size(); ++i) joined += (i ? "\n" : "") + names[i];
  return joined;
}
// node_names: every node's name joined by '\n' (the root's first); origin [n_rows][n_windows], age [leaves][n_windows]
EPVH_API int epvh_write_lineage_origins(const char *file, const char *node_names, uint64_t n_rows,
                                        const uint32_t *leaf_node, const uint32_t *branch_node, uint64_t n_windows,
                                        uint64_t window, int scale_exp, const uint64_t *origin, const uint64_t *age,
                                        uint64_t n_samples) {
  try {
    epv::write_lineage_origins(file, split_names(node_names), n_rows, leaf_node, branch_node, n_windows, window, scale_exp,
                               origin, age, n_samples);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_lineage_origins(const char *file) {
  try {
    return new epv::LineageOrigins(epv::read_lineage_origins(file));
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
// names_len: the bytes epvh_lineage_origins_copy needs for either list of names, the closing 0 included
EPVH_API void epvh_lineage_origins_dims(void *h, uint64_t *n_samples, uint64_t *window, uint64_t *n_windows, int *scale_exp,
                                        uint64_t *n_rows, uint64_t *n_leaves, uint64_t *names_len) {
  const epv::LineageOrigins *lo = (const epv::LineageOrigins *)h;
  *n_samples = lo->n_samples;
  *window = lo->window;
  *n_windows = lo->n_windows;
  *scale_exp = lo->scale_exp;
  *n_rows = lo->row_leaf.size();
  *n_leaves = lo->n_windows ? lo->age.size() / lo->n_windows : 0u;
  *names_len = std::max(join_names(lo->row_leaf).size(), join_names(lo->row_node).size()) + 1u;
}
EPVH_API void epvh_lineage_origins_copy(void *h, char *row_leaf, char *row_node, int names_len, uint64_t *origin,
                                        uint64_t *age) {
  const epv::LineageOrigins *lo = (const epv::LineageOrigins *)h;
  put_text(join_names(lo->row_leaf), row_leaf, names_len);
  put_text(join_names(lo->row_node), row_node, names_len);
  std::copy(lo->origin.begin(), lo->origin.end(), origin);
  std::copy(lo->age.begin(), lo->age.end(), age);
}
EPVH_API void epvh_lineage_origins_free(void *h) { delete (epv::LineageOrigins *)h; }

// ---- domain size spectra: bins, merge and close of parts (epv_domains.hpp), the file of epievo_est_histories -d
EPVH_API uint32_t epvh_domain_bin(uint64_t l) { return epv_domain_bin(l); }
EPVH_API void epvh_domain_bin_range(uint32_t b, uint64_t *lo, uint64_t *hi) { epv::domain_bin_range(b, lo, hi); }
// hists, len_sums, edges: n_parts pointers each, parts in genome order ([N][2][128], [N][2], [samples][N][2])
EPVH_API int epvh_domain_parts_merge(uint64_t n_parts, uint32_t N, uint64_t samples, const uint64_t *const *hists,
                                     const uint64_t *const *len_sums, const uint64_t *const *edges, uint64_t *out_hist,
                                     uint64_t *out_len_sum, uint64_t *out_edges) {
  try {
    epv::domain_parts_merge(n_parts, N, samples, hists, len_sums, edges, out_hist, out_len_sum, out_edges);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API int epvh_domain_part_close(uint32_t N, uint64_t samples, uint64_t *hist, uint64_t *len_sum, const uint64_t *edges) {
  try {
    epv::domain_part_close(N, samples, hist, len_sum, edges);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
// node_names: every node's name joined by '\n' (the root's first); hist [N][2][128], len_sum [N][2]: the closed result
EPVH_API int epvh_write_domain_stats(const char *file, const char *node_names, uint64_t n_samples, const uint64_t *hist,
                                     const uint64_t *len_sum) {
  try {
    epv::write_domain_stats(file, split_names(node_names), n_samples, hist, len_sum);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_domain_stats(const char *file) {
  try {
    return new epv::DomainStats(epv::read_domain_stats(file));
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
EPVH_API void epvh_domain_stats_dims(void *h, uint64_t *n_samples, uint64_t *n_nodes, uint64_t *names_len) {
  const epv::DomainStats *ds = (const epv::DomainStats *)h;
  *n_samples = ds->n_samples;
  *n_nodes = ds->node_names.size();
  *names_len = join_names(ds->node_names).size() + 1u;
}
EPVH_API void epvh_domain_stats_copy(void *h, char *names, int names_len, uint64_t *hist, uint64_t *len_sum) {
  const epv::DomainStats *ds = (const epv::DomainStats *)h;
  put_text(join_names(ds->node_names), names, names_len);
  std::copy(ds->hist.begin(), ds->hist.end(), hist);
  std::copy(ds->len_sum.begin(), ds->len_sum.end(), len_sum);
}
EPVH_API void epvh_domain_stats_free(void *h) { delete (epv::DomainStats *)h; }

// ---- domain turnover: merge and close of parts (epv_turnover.hpp), the file of epievo_est_histories -R
// hists, len_sums, edges: n_parts pointers each, parts in genome order ([R][2][2][128], [R][2][2], [samples][R][2])
EPVH_API int epvh_turnover_parts_merge(uint64_t n_parts, uint32_t R, uint64_t samples, const uint64_t *const *hists,
                                       const uint64_t *const *len_sums, const uint64_t *const *edges, uint64_t *out_hist,
                                       uint64_t *out_len_sum, uint64_t *out_edges) {
  try {
    epv::turnover_parts_merge(n_parts, R, samples, hists, len_sums, edges, out_hist, out_len_sum, out_edges);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API int epvh_turnover_part_close(uint32_t R, uint64_t samples, uint64_t *hist, uint64_t *len_sum, const uint64_t *edges) {
  try {
    epv::turnover_part_close(R, samples, hist, len_sum, edges);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
// branch_names: the child node's name of every branch joined by '\n'; hist [2 B][2][2][128], len_sum [2 B][2][2]: closed
EPVH_API int epvh_write_domain_turnover(const char *file, const char *branch_names, uint64_t n_samples, const uint64_t *hist,
                                        const uint64_t *len_sum) {
  try {
    epv::write_domain_turnover(file, split_names(branch_names), n_samples, hist, len_sum);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_domain_turnover(const char *file) {
  try {
    return new epv::DomainTurnover(epv::read_domain_turnover(file));
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
EPVH_API void epvh_domain_turnover_dims(void *h, uint64_t *n_samples, uint64_t *n_branches, uint64_t *names_len) {
  const epv::DomainTurnover *dt = (const epv::DomainTurnover *)h;
  *n_samples = dt->n_samples;
  *n_branches = dt->branch_names.size();
  *names_len = join_names(dt->branch_names).size() + 1u;
}
EPVH_API void epvh_domain_turnover_copy(void *h, char *names, int names_len, uint64_t *hist, uint64_t *len_sum) {
  const epv::DomainTurnover *dt = (const epv::DomainTurnover *)h;
  put_text(join_names(dt->branch_names), names, names_len);
  std::copy(dt->hist.begin(), dt->hist.end(), hist);
  std::copy(dt->len_sum.begin(), dt->len_sum.end(), len_sum);
}
EPVH_API void epvh_domain_turnover_free(void *h) { delete (epv::DomainTurnover *)h; }

// ---- change tracts: merge and close of parts (epv_tracts.hpp), the file of epievo_est_histories -X
// hists, len_sums, edges: n_parts pointers each, parts in genome order ([B][27][128], [B][27], [samples][B][2])
EPVH_API int epvh_tract_parts_merge(uint64_t n_parts, uint32_t B, uint64_t samples, const uint64_t *const *hists,
                                    const uint64_t *const *len_sums, const uint64_t *const *edges, uint64_t *out_hist,
                                    uint64_t *out_len_sum, uint64_t *out_edges) {
  try {
    epv::tract_parts_merge(n_parts, B, samples, hists, len_sums, edges, out_hist, out_len_sum, out_edges);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API int epvh_tract_part_close(uint32_t B, uint64_t samples, uint64_t *hist, uint64_t *len_sum, const uint64_t *edges) {
  try {
    epv::tract_part_close(B, samples, hist, len_sum, edges);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
// branch_names: the child node's name of every branch joined by '\n'; hist [B][27][128], len_sum [B][27]: closed
EPVH_API int epvh_write_change_tracts(const char *file, const char *branch_names, uint64_t n_samples, const uint64_t *hist,
                                      const uint64_t *len_sum) {
  try {
    epv::write_change_tracts(file, split_names(branch_names), n_samples, hist, len_sum);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_change_tracts(const char *file) {
  try {
    return new epv::ChangeTracts(epv::read_change_tracts(file));
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
EPVH_API void epvh_change_tracts_dims(void *h, uint64_t *n_samples, uint64_t *n_branches, uint64_t *names_len) {
  const epv::ChangeTracts *ct = (const epv::ChangeTracts *)h;
  *n_samples = ct->n_samples;
  *n_branches = ct->branch_names.size();
  *names_len = join_names(ct->branch_names).size() + 1u;
}
EPVH_API void epvh_change_tracts_copy(void *h, char *names, int names_len, uint64_t *hist, uint64_t *len_sum) {
  const epv::ChangeTracts *ct = (const epv::ChangeTracts *)h;
  put_text(join_names(ct->branch_names), names, names_len);
  std::copy(ct->hist.begin(), ct->hist.end(), hist);
  std::copy(ct->len_sum.begin(), ct->len_sum.end(), len_sum);
}
EPVH_API void epvh_change_tracts_free(void *h) { delete (epv::ChangeTracts *)h; }

// ---- spatial correlations: merge and close of parts (epv_corr.hpp), the file of epievo_est_histories -C
// cnts, n11s, edges: n_parts entries each, parts in genome order ([R][L + 1], [samples][R][2][LW]); out_cnt: the
// sites of the union
EPVH_API int epvh_corr_parts_merge(uint64_t n_parts, uint32_t R, uint32_t L, uint64_t samples, const uint64_t *cnts,
                                   const uint64_t *const *n11s, const uint64_t *const *edges, uint64_t *out_n11,
                                   uint64_t *out_edges, uint64_t *out_cnt) {
  try {
    const uint64_t n = epv::corr_parts_merge(n_parts, R, L, samples, cnts, n11s, edges, out_n11, out_edges);
    if (out_cnt) *out_cnt = n;
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API int epvh_corr_part_close(uint32_t R, uint32_t L, uint64_t samples, uint64_t n, const uint64_t *n11,
                                  const uint64_t *edges, uint64_t *left1, uint64_t *right1) {
  try {
    epv::corr_part_close(R, L, samples, n, n11, edges, left1, right1);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
// node_names: the N node names joined by '\n'; n11, left1, right1 [2 N - 1][L + 1]: closed
EPVH_API int epvh_write_spatial_correlation(const char *file, const char *node_names, uint64_t n_samples, uint64_t n_sites,
                                            uint32_t max_lag, const uint64_t *n11, const uint64_t *left1,
                                            const uint64_t *right1) {
  try {
    epv::write_spatial_correlation(file, split_names(node_names), n_samples, n_sites, max_lag, n11, left1, right1);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_spatial_correlation(const char *file) {
  try {
    return new epv::SpatialCorrelation(epv::read_spatial_correlation(file));
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
EPVH_API void epvh_spatial_correlation_dims(void *h, uint64_t *n_samples, uint64_t *n_sites, uint64_t *max_lag,
                                            uint64_t *n_rows, uint64_t *names_len) {
  const epv::SpatialCorrelation *sc = (const epv::SpatialCorrelation *)h;
  *n_samples = sc->n_samples;
  *n_sites = sc->n_sites;
  *max_lag = sc->max_lag;
  *n_rows = sc->row_names.size();
  *names_len = join_names(sc->row_names).size() + 1u;
}
EPVH_API void epvh_spatial_correlation_copy(void *h, char *names, int names_len, uint64_t *n11, uint64_t *left1,
                                            uint64_t *right1) {
  const epv::SpatialCorrelation *sc = (const epv::SpatialCorrelation *)h;
  put_text(join_names(sc->row_names), names, names_len);
  std::copy(sc->n11.begin(), sc->n11.end(), n11);
  std::copy(sc->left1.begin(), sc->left1.end(), left1);
  std::copy(sc->right1.begin(), sc->right1.end(), right1);
}
EPVH_API void epvh_spatial_correlation_free(void *h) { delete (epv::SpatialCorrelation *)h; }

// ---- domain maps: the membership rule, the CPU twin of the kernel and the merge of parts (epv_dmaps.hpp), the
// file of epievo_est_histories -D
EPVH_API int epvh_domain_map_members(const uint64_t *x, uint64_t nbits, uint32_t L, uint64_t *out) {
  try {
    epv::domain_map_members(x, nbits, L, out);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
// bits [N][ceil(cnt / 64)]; counts [N][K][cnt] receives + 1 per membership, edges [N][2][EW] this sample's records
EPVH_API int epvh_domain_maps_part(uint32_t N, uint32_t K, const uint32_t *sizes, uint64_t cnt, const uint64_t *bits,
                                   uint32_t *counts, uint64_t *edges) {
  try {
    epv::domain_maps_part(N, K, sizes, cnt, bits, counts, edges);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
// cnts, counts, edges: n_parts entries each, parts in genome order ([N][K][cnt], [samples][N][2][EW]); out_cnt: the
// sites of the union
EPVH_API int epvh_domain_maps_merge(uint64_t n_parts, uint32_t N, uint32_t K, const uint32_t *sizes, uint64_t samples,
                                    const uint64_t *cnts, const uint32_t *const *counts, const uint64_t *const *edges,
                                    uint32_t *out_counts, uint64_t *out_edges, uint64_t *out_cnt) {
  try {
    const uint64_t n = epv::domain_maps_merge(n_parts, N, K, sizes, samples, cnts, counts, edges, out_counts, out_edges);
    if (out_cnt) *out_cnt = n;
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
// node_names: the N node names joined by '\n'; sums [N][K][ceil(n_sites / W)]
EPVH_API int epvh_write_domain_maps(const char *file, const char *node_names, uint64_t n_samples, uint32_t state,
                                    uint32_t K, const uint32_t *sizes, uint64_t n_sites, uint64_t W, const uint64_t *sums) {
  try {
    epv::write_domain_maps(file, split_names(node_names), n_samples, state, std::vector<uint32_t>(sizes, sizes + K),
                           n_sites, W, sums);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_domain_maps(const char *file) {
  try {
    return new epv::DomainMaps(epv::read_domain_maps(file));
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
// words: samples, sites, window, state, nodes, K, length of the joined names with its terminator
EPVH_API void epvh_domain_maps_dims(void *h, uint64_t *words) {
  const epv::DomainMaps *dm = (const epv::DomainMaps *)h;
  words[0] = dm->n_samples;
  words[1] = dm->n_sites;
  words[2] = dm->window;
  words[3] = dm->state;
  words[4] = dm->node_names.size();
  words[5] = dm->sizes.size();
  words[6] = join_names(dm->node_names).size() + 1u;
}
EPVH_API void epvh_domain_maps_copy(void *h, char *names, int names_len, uint32_t *sizes, uint64_t *sums) {
  const epv::DomainMaps *dm = (const epv::DomainMaps *)h;
  put_text(join_names(dm->node_names), names, names_len);
  std::copy(dm->sizes.begin(), dm->sizes.end(), sizes);
  std::copy(dm->sums.begin(), dm->sums.end(), sums);
}
EPVH_API void epvh_domain_maps_free(void *h) { delete (epv::DomainMaps *)h; }

// ---- epoch statistics: closing the difference form (epv_epochs.hpp), and the file of epievo_est_histories -E
EPVH_API void epvh_epoch_edges(uint64_t fixT, uint32_t P, uint64_t *out) { epv::epoch_edges(fixT, P, out); }
EPVH_API int epvh_epoch_close(const uint64_t *raw, const uint64_t *fixT, uint32_t B, uint32_t P, uint64_t *closed) {
  try {
    epv::epoch_close(raw, fixT, B, P, closed);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
// closed[B][P][24], k[B] -> J, D[B][P][8] per sample
EPVH_API int epvh_epoch_counts_to_stats(const uint64_t *closed, const int *k, uint32_t B, uint32_t P, uint64_t samples,
                                        double *J, double *D) {
  try {
    epv::epoch_counts_to_stats(closed, k, B, P, samples, J, D);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
// node_names: n_nodes names joined by '\n' (the root's first); branch_len, scale_exp, fixT: [n_nodes], index 0 = root
EPVH_API int epvh_write_epoch_stats(const char *file, const char *node_names, int n_nodes, uint32_t P,
                                    const double *branch_len, const int *scale_exp, const uint64_t *fixT,
                                    const uint64_t *closed, uint64_t n_samples, const double *rates) {
  try {
    std::vector<std::string> names;
    std::string all(node_names), cur;
    for (char ch : all) {
      if (ch == '\n') { names.push_back(cur); cur.clear(); } else cur.push_back(ch);
    }
    names.push_back(cur);
    if ((int)names.size() != n_nodes) throw std::runtime_error("epvh_write_epoch_stats: one name per node");
    std::array<double, 8> r;
    for (int i = 0; i < 8; ++i) r[i] = rates[i];
    epv::write_epoch_stats(file, names, n_nodes, P, branch_len, scale_exp, fixT, closed, n_samples, r);
    return 0;
  } catch (const std::exception &e) { g_err = e.what(); return 1; }
}
EPVH_API void *epvh_read_epoch_stats(const char *file) {
  try {
    return new epv::EpochStats(epv::read_epoch_stats(file));
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}
static std::string joined_names(const epv::EpochStats *es) {
  std::string joined;
  for (size_t i = 0; i < es->node_names.size(); ++i) joined += (i ? "\n" : "") + es->node_names[i];
  return joined;
}
// names_len: the bytes epvh_epoch_stats_copy needs for the names, the closing 0 included
EPVH_API void epvh_epoch_stats_dims(void *h, uint64_t *n_samples, uint64_t *n_epochs, uint64_t *n_branches,
                                    uint64_t *names_len) {
  const epv::EpochStats *es = (const epv::EpochStats *)h;
  *names_len = joined_names(es).size() + 1u;
  *n_samples = es->n_samples;
  *n_epochs = es->n_epochs;
  *n_branches = es->node_names.size();
}
// names: the non-root nodes' names joined by '\n'; branch_len, scale_exp: [B]; closed [B][P][24]; start, factor [B][P]
EPVH_API void epvh_epoch_stats_copy(void *h, char *names, int names_len, double *branch_len, int *scale_exp,
                                    uint64_t *closed, double *start, double *factor) {
  const epv::EpochStats *es = (const epv::EpochStats *)h;
  put_text(joined_names(es), names, names_len);
  std::copy(es->branch_len.begin(), es->branch_len.end(), branch_len);
  std::copy(es->scale_exp.begin(), es->scale_exp.end(), scale_exp);
  std::copy(es->closed.begin(), es->closed.end(), closed);
  std::copy(es->start.begin(), es->start.end(), start);
  std::copy(es->factor.begin(), es->factor.end(), factor);
}
EPVH_API void epvh_epoch_stats_free(void *h) { delete (epv::EpochStats *)h; }

// ---- the plan of a colour phase without a GPU: epv_plan.h, which the device library decides with.  The tree as
// epv_set_tree takes it (checked by the same pre-order rules), the local sites, the jump capacity and the mean jumps
// per (site, branch) as a context holds them, the option word as epv_set_options accepts it, the counts of
// unobserved and evidence leaf cells, and the knobs as n_knobs strings NAME=VALUE in place of the environment.
// *word: what epv_phase_plan reports for such a context
// *word: what epv_phase_plan reports for such a context.  p2 (may be null): the launch shape of the second proposal
// kernel and of the fused phase in its buffers (plan_p2) -- planned, fused, pool doubles per wave, dynamic LDS bytes,
// sites per fused wave
EPVH_API int epvh_phase_plan2(int n_nodes, const uint32_t *parent_ids, const uint32_t *subtree_sizes, uint64_t n_sites,
                              uint32_t capacity, double kbar, uint32_t options, uint64_t unobs_cells,
                              uint64_t evidence_cells, const char *const *knobs, int n_knobs, uint32_t *word,
                              uint64_t p2[5]) {
  if (n_nodes < 2 || n_nodes > 4095 || !parent_ids || !subtree_sizes || !word || n_knobs < 0 || (n_knobs && !knobs)) {
    g_err = "bad tree";
    return 1;
  }
  for (int i = 1; i < n_nodes; ++i)
    if (parent_ids[i] >= (uint32_t)i || subtree_sizes[i] < 1 || i + subtree_sizes[i] > (uint32_t)n_nodes) {
      g_err = "tree arrays are not a valid pre-order tree";
      return 1;
    }
  if (n_sites < 3 || capacity < 1 || capacity > EPV_MAX_CAP || !(kbar >= 0.0)) {
    g_err = "bad paths: at least 3 sites, a capacity of 1 .. 2047, a mean jump count >= 0";
    return 1;
  }
  const EpvKnobs k = read_knobs([&](const char *name) -> const char * {
    const size_t len = std::strlen(name);
    for (int i = 0; i < n_knobs; ++i)
      if (knobs[i] && !std::strncmp(knobs[i], name, len) && knobs[i][len] == '=') return knobs[i] + len + 1;
    return nullptr;
  });
  const PhaseShapes shapes = plan_shapes({(uint32_t)n_nodes, parent_ids, subtree_sizes, capacity, n_sites, kbar}, k);
  if (shapes.error) {
    g_err = shapes.error;
    return 1;
  }
  *word = phase_plan(shapes, k, options, unobs_cells, evidence_cells, (uint32_t)n_nodes - 1u, kbar).word();
  if (p2) {
    const PlanV2 &v = shapes.v2;
    p2[0] = v.planned ? 1u : 0u; p2[1] = v.fused ? 1u : 0u; p2[2] = v.pool; p2[3] = v.lds; p2[4] = v.fused_lanes;
  }
  return 0;
}
EPVH_API int epvh_phase_plan(int n_nodes, const uint32_t *parent_ids, const uint32_t *subtree_sizes, uint64_t n_sites,
                             uint32_t capacity, double kbar, uint32_t options, uint64_t unobs_cells,
                             uint64_t evidence_cells, const char *const *knobs, int n_knobs, uint32_t *word) {
  return epvh_phase_plan2(n_nodes, parent_ids, subtree_sizes, n_sites, capacity, kbar, options, unobs_cells, evidence_cells,
                          knobs, n_knobs, word, nullptr);
}
