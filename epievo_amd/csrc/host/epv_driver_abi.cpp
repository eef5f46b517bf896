// epv_driver_abi.cpp -- include/epievo_mi355x_driver.h: a flat C face over epv::SingleSiteSampler so
// that bench.py and the tests drive the product's C++ EM driver (epv_sampler.cpp + libepv_rccl.so).
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <memory>
#include <string>

#include "epievo_mi355x_comm.h"
#include "epievo_mi355x_driver.h"
#include "epv_sampler.hpp"

#define EPVD_API extern "C" __attribute__((visibility("default")))

struct epvd_sampler {
  std::unique_ptr<epv::SingleSiteSampler> s;
  bool rank_mode = false;
  std::string err;
  epv::FlatPaths staged;   // between epvd_download_sizes and epvd_download
  std::vector<uint32_t> staged_avg;   // between epvd_path_average_sizes and epvd_download_path_average
  bool have_staged_avg = false;
  std::vector<uint32_t> staged_events;   // between epvd_branch_events_sizes and epvd_download_branch_events
  bool have_staged_events = false;
  std::vector<uint32_t> staged_patterns;   // between epvd_change_patterns_sizes and epvd_download_change_patterns
  bool have_staged_patterns = false;
  std::vector<int64_t> staged_wstat;   // between epvd_window_stats_sizes and epvd_download_window_stats
  uint64_t staged_wstat_nw = 0, staged_wstat_ns = 0;
  bool have_staged_wstat = false;
  std::vector<uint64_t> staged_epoch;   // between epvd_epoch_stats_sizes and epvd_download_epoch_stats
  std::vector<int> staged_epoch_k;
  std::vector<uint64_t> staged_epoch_fixT;
  uint64_t staged_epoch_ns = 0;
  bool have_staged_epoch = false;
  std::vector<uint32_t> staged_origin;   // between epvd_lineage_origins_sizes and epvd_download_lineage_origins
  std::vector<uint64_t> staged_age;
  bool have_staged_origins = false;
  std::vector<uint64_t> staged_dom_hist, staged_dom_len, staged_dom_edges;   // between epvd_domain_part_sizes and epvd_download_domain_part
  bool have_staged_domains = false;
  std::vector<uint64_t> staged_turn_hist, staged_turn_len, staged_turn_edges;   // between epvd_turnover_part_sizes and epvd_download_turnover_part
  bool have_staged_turnover = false;
  std::vector<uint64_t> staged_tract_hist, staged_tract_len, staged_tract_edges;   // between epvd_tracts_part_sizes and epvd_download_tracts_part
  bool have_staged_tracts = false;
  std::vector<uint64_t> staged_corr_n11, staged_corr_edges;   // between epvd_corr_part_sizes and epvd_download_corr_part
  bool have_staged_corr = false;
  std::vector<uint32_t> staged_dmaps_counts;   // between epvd_dmaps_sizes and epvd_download_dmaps
  std::vector<uint64_t> staged_dmaps_edges;
  bool have_staged_dmaps = false;
  std::vector<uint64_t> staged_mix_words, staged_mix_sums;   // between epvd_mixing_sizes and epvd_download_mixing
  std::vector<uint32_t> staged_mix_moved;
  bool have_staged_mixing = false;
};

namespace {
thread_local std::string g_err;

epv::Model make_model(const double *rates, const double *T) {
  epv::Model m;
  for (int i = 0; i < 8; ++i) m.rates[i] = rates[i];
  for (int i = 0; i < 4; ++i) m.T[i] = T[i];
  return m;
}

template <class F>
int guarded(epvd_sampler *h, F &&f) {
  if (!h) return 1;
  try { f(); return 0; }
  catch (const std::exception &e) { h->err = e.what(); return 1; }
}
}  // namespace

EPVD_API epvd_sampler *epvd_create(uint64_t burn_in, uint64_t batch, int n_devices, const int *devices, uint32_t capacity) {
  try {
    std::unique_ptr<epvd_sampler> h(new epvd_sampler());
    std::vector<int> devs(devices, devices + (n_devices > 0 ? n_devices : 0));
    h->s.reset(new epv::SingleSiteSampler(burn_in, batch, devs, capacity));
    return h.release();
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}

EPVD_API int epvd_unique_id(void *id128) { return epv_comm_get_unique_id(id128); }

EPVD_API epvd_sampler *epvd_create_rank(uint64_t burn_in, uint64_t batch, int device, int world, int rank,
                                        const void *id128, uint32_t capacity) {
  try {
    if (!id128) throw std::runtime_error("null communicator id");
    std::unique_ptr<epvd_sampler> h(new epvd_sampler());
    epv::RankSpec r;
    r.device = device; r.world = world; r.rank = rank;
    std::memcpy(r.id, id128, sizeof r.id);
    h->s.reset(new epv::SingleSiteSampler(burn_in, batch, r, capacity));
    h->rank_mode = true;
    return h.release();
  } catch (const std::exception &e) { g_err = e.what(); return nullptr; }
}

EPVD_API void epvd_destroy(epvd_sampler *h) { delete h; }
EPVD_API const char *epvd_last_error(const epvd_sampler *h) { return h ? h->err.c_str() : g_err.c_str(); }

EPVD_API int epvd_shard_cuts(uint64_t n_sites, int world, uint64_t burn_in, uint64_t batch, uint64_t *cuts) {
  if (!cuts || world < 1) return 0;
  const std::vector<uint64_t> c = epv::SingleSiteSampler::shard_cuts(n_sites, (size_t)world, burn_in, batch);
  for (size_t i = 0; i < c.size(); ++i) cuts[i] = c[i];
  return (int)c.size() - 1;
}

EPVD_API int epvd_reset(epvd_sampler *h, const double *rates, const double *T, int n_nodes, const uint32_t *parent_ids,
                        const uint32_t *subtree_sizes, const double *branches, uint64_t n_sites, const uint8_t *init_state,
                        const uint64_t *offsets, const double *jumps, uint64_t n_global) {
  return guarded(h, [&] {
    epv::Tree th;
    th.subtree_sizes.assign(subtree_sizes, subtree_sizes + n_nodes);
    th.parent_ids.assign(parent_ids, parent_ids + n_nodes);
    th.branches.assign(branches, branches + n_nodes);
    th.node_names.resize(n_nodes);
    th.name_generated.assign(n_nodes, true);
    epv::FlatPaths fp;
    fp.n_sites = n_sites;
    fp.n_nodes = n_nodes;
    const uint64_t E = (uint64_t)(n_nodes - 1) * n_sites;
    fp.init.assign(init_state, init_state + E);
    fp.offsets.assign(offsets, offsets + E + 1);
    fp.jumps.assign(jumps, jumps + offsets[E]);
    if (h->rank_mode) h->s->reset(make_model(rates, T), th, fp, n_global ? n_global : n_sites);
    else h->s->reset(make_model(rates, T), th, fp);
  });
}

EPVD_API int epvd_reset_model(epvd_sampler *h, const double *rates, const double *T) {
  return guarded(h, [&] { h->s->reset(make_model(rates, T)); });
}

EPVD_API int epvd_run_mcmc(epvd_sampler *h, uint64_t seed, uint64_t em_iteration, double *J, double *D, double *acc_rate) {
  return guarded(h, [&] {
    std::vector<std::vector<double>> Jv, Dv;
    double acc = 0.0;
    h->s->run_mcmc(seed, em_iteration, Jv, Dv, acc);
    for (size_t b = 1; b < Jv.size(); ++b)
      for (int k = 0; k < 8; ++k) { J[(b - 1) * 8 + k] = Jv[b][k]; D[(b - 1) * 8 + k] = Dv[b][k]; }
    if (acc_rate) *acc_rate = acc;
  });
}

EPVD_API int epvd_scale_jump_times(epvd_sampler *h, const double *new_branches, int n_nodes) {
  return guarded(h, [&] { h->s->scale_jump_times(std::vector<double>(new_branches, new_branches + n_nodes)); });
}

EPVD_API int epvd_download_sizes(epvd_sampler *h, uint64_t *n_sites, uint64_t *total_jumps) {
  return guarded(h, [&] {
    h->s->download(h->staged);
    *n_sites = h->staged.n_sites;
    *total_jumps = h->staged.jumps.size();
  });
}

EPVD_API int epvd_download(epvd_sampler *h, uint8_t *init_state, uint64_t *offsets, double *jumps) {
  return guarded(h, [&] {
    const epv::FlatPaths &p = h->staged;
    if (p.offsets.empty()) throw std::runtime_error("epvd_download_sizes first");
    std::copy(p.init.begin(), p.init.end(), init_state);
    std::copy(p.offsets.begin(), p.offsets.end(), offsets);
    std::copy(p.jumps.begin(), p.jumps.end(), jumps);
    h->staged = epv::FlatPaths();
  });
}

EPVD_API int epvd_layout(epvd_sampler *h, char *buf, int len, int *n_slots_here, int *n_parts_here, int *uses_rccl,
                         uint64_t *halo_columns) {
  return guarded(h, [&] {
    if (buf && len > 0) { std::strncpy(buf, h->s->layout().c_str(), (size_t)len - 1); buf[len - 1] = '\0'; }
    if (n_slots_here) *n_slots_here = (int)h->s->n_slots();
    if (n_parts_here) *n_parts_here = (int)h->s->n_parts();
    if (uses_rccl) *uses_rccl = h->s->uses_rccl() ? 1 : 0;
    if (halo_columns) *halo_columns = h->s->halo_columns();
  });
}

EPVD_API int epvd_set_options(epvd_sampler *h, uint32_t flags) { return guarded(h, [&] { h->s->set_options(flags); }); }
EPVD_API int epvd_set_timing(epvd_sampler *h, int every) { return guarded(h, [&] { h->s->set_timing(every); }); }
EPVD_API int epvd_kernel_time_ms(epvd_sampler *h, double *avg_ms, uint64_t *n_launches) {
  return guarded(h, [&] { h->s->kernel_time_ms(*avg_ms, *n_launches); });
}
EPVD_API int epvd_phase_mode(epvd_sampler *h, uint32_t *mode) { return guarded(h, [&] { *mode = h->s->phase_mode(); }); }
EPVD_API int epvd_set_unobserved(epvd_sampler *h, uint64_t n_sites, int n_nodes, const uint8_t *unobserved) {
  return guarded(h, [&] {
    std::vector<uint8_t> m;
    if (unobserved) m.assign(unobserved, unobserved + (uint64_t)(n_nodes - 1) * n_sites);
    h->s->set_unobserved(std::move(m));
  });
}

EPVD_API int epvd_set_regions(epvd_sampler *h, uint64_t n_regions, const uint64_t *lengths) {
  return guarded(h, [&] {
    std::vector<uint64_t> m;
    if (lengths) m.assign(lengths, lengths + n_regions);
    h->s->set_regions(std::move(m));
  });
}

EPVD_API int epvd_set_leaf_evidence(epvd_sampler *h, uint64_t n_sites, int n_nodes, const float *p_state1) {
  return guarded(h, [&] {
    std::vector<float> r;
    if (p_state1) r.assign(p_state1, p_state1 + (uint64_t)(n_nodes - 1) * n_sites);
    h->s->set_leaf_evidence(std::move(r));
  });
}

EPVD_API int epvd_set_path_average(epvd_sampler *h, uint32_t n_points) {
  return guarded(h, [&] { h->s->set_path_average(n_points); });
}
EPVD_API int epvd_path_average_sizes(epvd_sampler *h, uint64_t *n_values, uint32_t *n_points, uint64_t *n_samples) {
  return guarded(h, [&] {
    uint64_t ns = 0;
    h->s->download_path_average(h->staged_avg, ns);
    h->have_staged_avg = true;
    *n_values = h->staged_avg.size();
    *n_points = h->s->path_average_points();
    *n_samples = ns;
  });
}
EPVD_API int epvd_download_path_average(epvd_sampler *h, uint32_t *counts) {
  return guarded(h, [&] {
    if (!h->have_staged_avg) throw std::runtime_error("epvd_path_average_sizes first");
    std::copy(h->staged_avg.begin(), h->staged_avg.end(), counts);
    h->staged_avg.clear();
    h->have_staged_avg = false;
  });
}

EPVD_API int epvd_set_branch_events(epvd_sampler *h, int on) {
  return guarded(h, [&] { h->s->set_branch_events(on != 0); });
}
EPVD_API int epvd_branch_events_sizes(epvd_sampler *h, uint64_t *n_values, uint64_t *n_samples) {
  return guarded(h, [&] {
    uint64_t ns = 0;
    h->s->download_branch_events(h->staged_events, ns);
    h->have_staged_events = true;
    *n_values = h->staged_events.size();
    *n_samples = ns;
  });
}
EPVD_API int epvd_download_branch_events(epvd_sampler *h, uint32_t *planes) {
  return guarded(h, [&] {
    if (!h->have_staged_events) throw std::runtime_error("epvd_branch_events_sizes first");
    std::copy(h->staged_events.begin(), h->staged_events.end(), planes);
    h->staged_events.clear();
    h->have_staged_events = false;
  });
}
EPVD_API int epvd_download_branch_event_windows(epvd_sampler *h, uint64_t W, uint64_t n_windows, uint64_t *sums,
                                                uint64_t *n_samples) {
  return guarded(h, [&] {
    std::vector<uint64_t> v;
    uint64_t ns = 0;
    if (n_windows != h->s->branch_event_windows(W))
      throw std::runtime_error("epvd_download_branch_event_windows: n_windows must be ceil(genome length / W), W >= 1");
    h->s->download_branch_event_windows(W, v, ns);
    std::copy(v.begin(), v.end(), sums);
    if (n_samples) *n_samples = ns;
  });
}

EPVD_API int epvd_set_mixing(epvd_sampler *h, uint32_t max_lag) {
  return guarded(h, [&] { h->s->enable_mixing(max_lag); });
}
EPVD_API int epvd_mixing_sizes(epvd_sampler *h, uint64_t *n_sites, uint32_t *max_lag) {
  return guarded(h, [&] {
    h->s->download_mixing(h->staged_mix_words, h->staged_mix_moved, h->staged_mix_sums);
    h->have_staged_mixing = true;
    *n_sites = h->staged_mix_moved.size();
    *max_lag = h->s->mixing_max_lag();
  });
}
EPVD_API int epvd_download_mixing(epvd_sampler *h, uint64_t *words, uint32_t *moved, uint64_t *sums) {
  return guarded(h, [&] {
    if (!h->have_staged_mixing) throw std::runtime_error("epvd_mixing_sizes first");
    std::copy(h->staged_mix_words.begin(), h->staged_mix_words.end(), words);
    std::copy(h->staged_mix_moved.begin(), h->staged_mix_moved.end(), moved);
    std::copy(h->staged_mix_sums.begin(), h->staged_mix_sums.end(), sums);
    h->staged_mix_words.clear(); h->staged_mix_moved.clear(); h->staged_mix_sums.clear();
    h->have_staged_mixing = false;
  });
}

EPVD_API int epvd_set_change_patterns(epvd_sampler *h, int on) {
  return guarded(h, [&] { h->s->set_change_patterns(on != 0); });
}
EPVD_API int epvd_change_patterns_sizes(epvd_sampler *h, uint64_t *n_values, uint32_t *n_rows, uint64_t *n_samples) {
  return guarded(h, [&] {
    uint64_t ns = 0;
    uint32_t R = 0;
    h->s->download_change_patterns(h->staged_patterns, R, ns);
    h->have_staged_patterns = true;
    *n_values = h->staged_patterns.size();
    *n_rows = R;
    *n_samples = ns;
  });
}
EPVD_API int epvd_download_change_patterns(epvd_sampler *h, uint32_t *rows) {
  return guarded(h, [&] {
    if (!h->have_staged_patterns) throw std::runtime_error("epvd_change_patterns_sizes first");
    std::copy(h->staged_patterns.begin(), h->staged_patterns.end(), rows);
    h->staged_patterns.clear();
    h->have_staged_patterns = false;
  });
}
EPVD_API int epvd_download_change_pattern_windows(epvd_sampler *h, uint64_t W, uint32_t n_rows, uint64_t n_windows,
                                                  uint64_t *sums, uint64_t *n_samples) {
  return guarded(h, [&] {
    std::vector<uint64_t> v;
    uint64_t ns = 0;
    uint32_t R = 0;
    if (n_windows != h->s->branch_event_windows(W))
      throw std::runtime_error("epvd_download_change_pattern_windows: n_windows must be ceil(genome length / W), W >= 1");
    h->s->download_change_pattern_windows(W, v, R, ns);
    if (R != n_rows) throw std::runtime_error("epvd_download_change_pattern_windows: n_rows must be the rows of epvd_change_patterns_sizes");
    std::copy(v.begin(), v.end(), sums);
    if (n_samples) *n_samples = ns;
  });
}

EPVD_API int epvd_set_window_stats(epvd_sampler *h, uint64_t W) {
  return guarded(h, [&] { h->s->set_window_stats(W); });
}
EPVD_API int epvd_window_stats_sizes(epvd_sampler *h, uint64_t *W, uint64_t *n_windows, uint64_t *n_samples) {
  return guarded(h, [&] {
    uint64_t w = 0, nw = 0, ns = 0;
    h->s->download_window_stats(h->staged_wstat, w, nw, ns);
    h->have_staged_wstat = true;
    h->staged_wstat_nw = nw;
    h->staged_wstat_ns = ns;
    *W = w;
    *n_windows = nw;
    *n_samples = ns;
  });
}
EPVD_API int epvd_download_window_stats(epvd_sampler *h, int64_t *counts, double *J, double *D) {
  return guarded(h, [&] {
    if (!h->have_staged_wstat) throw std::runtime_error("epvd_window_stats_sizes first");
    if (counts) std::copy(h->staged_wstat.begin(), h->staged_wstat.end(), counts);
    if (J && D && h->staged_wstat_ns) {
      std::vector<double> j, d;
      h->s->window_counts_to_stats(h->staged_wstat, h->staged_wstat_nw, h->staged_wstat_ns, j, d);
      std::copy(j.begin(), j.end(), J);
      std::copy(d.begin(), d.end(), D);
    }
    h->staged_wstat.clear();
    h->have_staged_wstat = false;
  });
}

EPVD_API int epvd_set_lineage_origins(epvd_sampler *h, int on) {
  return guarded(h, [&] { h->s->set_lineage_origins(on != 0); });
}
EPVD_API int epvd_reset_lineage_origins(epvd_sampler *h) {
  return guarded(h, [&] { h->s->reset_lineage_origins(); });
}
EPVD_API int epvd_accumulate_lineage_origins(epvd_sampler *h) {
  return guarded(h, [&] { h->s->accumulate_lineage_origins(); });
}
EPVD_API int epvd_lineage_origin_rows(epvd_sampler *h, uint32_t *n_leaves, uint32_t *n_rows, uint32_t *leaf_node,
                                      uint32_t *branch_node) {
  return guarded(h, [&] {
    std::vector<uint32_t> leaf, node;
    h->s->lineage_origin_rows(leaf, node);
    uint32_t L = 0;
    for (uint32_t v : node) L += v == 0u;   // one root row per leaf
    *n_leaves = L;
    *n_rows = (uint32_t)node.size();
    if (leaf_node) std::copy(leaf.begin(), leaf.end(), leaf_node);
    if (branch_node) std::copy(node.begin(), node.end(), branch_node);
  });
}
EPVD_API int epvd_lineage_origins_scale_exp(epvd_sampler *h, int *k) {
  return guarded(h, [&] { *k = h->s->lineage_origins_scale_exp(); });
}
EPVD_API int epvd_lineage_origins_sizes(epvd_sampler *h, uint64_t *n_origin, uint64_t *n_age, int *k, uint64_t *n_samples) {
  return guarded(h, [&] {
    uint64_t ns = 0;
    int kk = 0;
    h->s->download_lineage_origins(h->staged_origin, h->staged_age, kk, ns);
    h->have_staged_origins = true;
    *n_origin = h->staged_origin.size();
    *n_age = h->staged_age.size();
    *k = kk;
    *n_samples = ns;
  });
}
EPVD_API int epvd_download_lineage_origins(epvd_sampler *h, uint32_t *origin, uint64_t *age) {
  return guarded(h, [&] {
    if (!h->have_staged_origins) throw std::runtime_error("epvd_lineage_origins_sizes first");
    std::copy(h->staged_origin.begin(), h->staged_origin.end(), origin);
    std::copy(h->staged_age.begin(), h->staged_age.end(), age);
    h->staged_origin.clear();
    h->staged_age.clear();
    h->have_staged_origins = false;
  });
}
EPVD_API int epvd_download_lineage_origin_windows(epvd_sampler *h, uint64_t W, uint64_t n_windows, uint64_t *origin,
                                                  uint64_t *age, int *k, uint64_t *n_samples) {
  return guarded(h, [&] {
    std::vector<uint64_t> o, a;
    uint64_t ns = 0;
    int kk = 0;
    if (n_windows != h->s->branch_event_windows(W))
      throw std::runtime_error("epvd_download_lineage_origin_windows: n_windows must be ceil(genome length / W), W >= 1");
    h->s->download_lineage_origin_windows(W, o, a, kk, ns);
    std::copy(o.begin(), o.end(), origin);
    std::copy(a.begin(), a.end(), age);
    if (k) *k = kk;
    if (n_samples) *n_samples = ns;
  });
}

EPVD_API int epvd_set_domain_stats(epvd_sampler *h, uint64_t max_samples) {
  return guarded(h, [&] { h->s->set_domain_stats(max_samples); });
}
EPVD_API int epvd_reset_domain_stats(epvd_sampler *h) {
  return guarded(h, [&] { h->s->reset_domain_stats(); });
}
EPVD_API int epvd_accumulate_domain_stats(epvd_sampler *h) {
  return guarded(h, [&] { h->s->accumulate_domain_stats(); });
}
EPVD_API int epvd_domain_part_sizes(epvd_sampler *h, uint32_t *n_nodes, uint64_t *n_samples) {
  return guarded(h, [&] {
    h->s->download_domain_part(h->staged_dom_hist, h->staged_dom_len, h->staged_dom_edges, *n_nodes, *n_samples);
    h->have_staged_domains = true;
  });
}
EPVD_API int epvd_download_domain_part(epvd_sampler *h, uint64_t *hist, uint64_t *len_sum, uint64_t *edges) {
  return guarded(h, [&] {
    if (!h->have_staged_domains) throw std::runtime_error("epvd_domain_part_sizes first");
    std::copy(h->staged_dom_hist.begin(), h->staged_dom_hist.end(), hist);
    std::copy(h->staged_dom_len.begin(), h->staged_dom_len.end(), len_sum);
    std::copy(h->staged_dom_edges.begin(), h->staged_dom_edges.end(), edges);
    h->staged_dom_hist.clear();
    h->staged_dom_len.clear();
    h->staged_dom_edges.clear();
    h->have_staged_domains = false;
  });
}
EPVD_API int epvd_download_domain_stats(epvd_sampler *h, uint32_t n_nodes, uint64_t *hist, uint64_t *len_sum,
                                        uint64_t *n_samples) {
  return guarded(h, [&] {
    std::vector<uint64_t> hh, ll;
    uint32_t N = 0;
    uint64_t ns = 0;
    h->s->download_domain_stats(hh, ll, N, ns);
    if (N != n_nodes) throw std::runtime_error("epvd_download_domain_stats: n_nodes must be the tree's number of nodes");
    std::copy(hh.begin(), hh.end(), hist);
    std::copy(ll.begin(), ll.end(), len_sum);
    if (n_samples) *n_samples = ns;
  });
}

EPVD_API int epvd_set_turnover(epvd_sampler *h, uint64_t max_samples) {
  return guarded(h, [&] { h->s->set_domain_turnover(max_samples); });
}
EPVD_API int epvd_reset_turnover(epvd_sampler *h) {
  return guarded(h, [&] { h->s->reset_domain_turnover(); });
}
EPVD_API int epvd_accumulate_turnover(epvd_sampler *h) {
  return guarded(h, [&] { h->s->accumulate_domain_turnover(); });
}
EPVD_API int epvd_turnover_part_sizes(epvd_sampler *h, uint32_t *n_rows, uint64_t *n_samples) {
  return guarded(h, [&] {
    h->s->download_domain_turnover_part(h->staged_turn_hist, h->staged_turn_len, h->staged_turn_edges, *n_rows, *n_samples);
    h->have_staged_turnover = true;
  });
}
EPVD_API int epvd_download_turnover_part(epvd_sampler *h, uint64_t *hist, uint64_t *len_sum, uint64_t *edges) {
  return guarded(h, [&] {
    if (!h->have_staged_turnover) throw std::runtime_error("epvd_turnover_part_sizes first");
    std::copy(h->staged_turn_hist.begin(), h->staged_turn_hist.end(), hist);
    std::copy(h->staged_turn_len.begin(), h->staged_turn_len.end(), len_sum);
    std::copy(h->staged_turn_edges.begin(), h->staged_turn_edges.end(), edges);
    h->staged_turn_hist.clear();
    h->staged_turn_len.clear();
    h->staged_turn_edges.clear();
    h->have_staged_turnover = false;
  });
}
EPVD_API int epvd_download_turnover(epvd_sampler *h, uint32_t n_rows, uint64_t *hist, uint64_t *len_sum,
                                    uint64_t *n_samples) {
  return guarded(h, [&] {
    std::vector<uint64_t> hh, ll;
    uint32_t R = 0;
    uint64_t ns = 0;
    h->s->download_domain_turnover(hh, ll, R, ns);
    if (R != n_rows) throw std::runtime_error("epvd_download_turnover: n_rows must be twice the tree's number of branches");
    std::copy(hh.begin(), hh.end(), hist);
    std::copy(ll.begin(), ll.end(), len_sum);
    if (n_samples) *n_samples = ns;
  });
}

EPVD_API int epvd_set_tracts(epvd_sampler *h, uint64_t max_samples) {
  return guarded(h, [&] { h->s->set_change_tracts(max_samples); });
}
EPVD_API int epvd_reset_tracts(epvd_sampler *h) {
  return guarded(h, [&] { h->s->reset_change_tracts(); });
}
EPVD_API int epvd_accumulate_tracts(epvd_sampler *h) {
  return guarded(h, [&] { h->s->accumulate_change_tracts(); });
}
EPVD_API int epvd_tracts_part_sizes(epvd_sampler *h, uint32_t *n_branches, uint64_t *n_samples) {
  return guarded(h, [&] {
    h->s->download_change_tracts_part(h->staged_tract_hist, h->staged_tract_len, h->staged_tract_edges, *n_branches, *n_samples);
    h->have_staged_tracts = true;
  });
}
EPVD_API int epvd_download_tracts_part(epvd_sampler *h, uint64_t *hist, uint64_t *len_sum, uint64_t *edges) {
  return guarded(h, [&] {
    if (!h->have_staged_tracts) throw std::runtime_error("epvd_tracts_part_sizes first");
    std::copy(h->staged_tract_hist.begin(), h->staged_tract_hist.end(), hist);
    std::copy(h->staged_tract_len.begin(), h->staged_tract_len.end(), len_sum);
    std::copy(h->staged_tract_edges.begin(), h->staged_tract_edges.end(), edges);
    h->staged_tract_hist.clear();
    h->staged_tract_len.clear();
    h->staged_tract_edges.clear();
    h->have_staged_tracts = false;
  });
}
EPVD_API int epvd_download_tracts(epvd_sampler *h, uint32_t n_branches, uint64_t *hist, uint64_t *len_sum,
                                  uint64_t *n_samples) {
  return guarded(h, [&] {
    std::vector<uint64_t> hh, ll;
    uint32_t B = 0;
    uint64_t ns = 0;
    h->s->download_change_tracts(hh, ll, B, ns);
    if (B != n_branches) throw std::runtime_error("epvd_download_tracts: n_branches must be the tree's number of branches");
    std::copy(hh.begin(), hh.end(), hist);
    std::copy(ll.begin(), ll.end(), len_sum);
    if (n_samples) *n_samples = ns;
  });
}

EPVD_API int epvd_set_corr(epvd_sampler *h, uint32_t max_lag, uint64_t max_samples) {
  return guarded(h, [&] { h->s->set_spatial_correlation(max_lag, max_samples); });
}
EPVD_API int epvd_reset_corr(epvd_sampler *h) {
  return guarded(h, [&] { h->s->reset_spatial_correlation(); });
}
EPVD_API int epvd_accumulate_corr(epvd_sampler *h) {
  return guarded(h, [&] { h->s->accumulate_spatial_correlation(); });
}
EPVD_API int epvd_corr_part_sizes(epvd_sampler *h, uint32_t *n_rows, uint32_t *max_lag, uint64_t *n_samples,
                                  uint64_t *n_sites) {
  return guarded(h, [&] {
    h->s->download_spatial_correlation_part(h->staged_corr_n11, h->staged_corr_edges, *n_rows, *max_lag, *n_samples,
                                            *n_sites);
    h->have_staged_corr = true;
  });
}
EPVD_API int epvd_download_corr_part(epvd_sampler *h, uint64_t *n11, uint64_t *edges) {
  return guarded(h, [&] {
    if (!h->have_staged_corr) throw std::runtime_error("epvd_corr_part_sizes first");
    std::copy(h->staged_corr_n11.begin(), h->staged_corr_n11.end(), n11);
    std::copy(h->staged_corr_edges.begin(), h->staged_corr_edges.end(), edges);
    h->staged_corr_n11.clear();
    h->staged_corr_edges.clear();
    h->have_staged_corr = false;
  });
}
EPVD_API int epvd_set_dmaps(epvd_sampler *h, uint32_t n_sizes, const uint32_t *sizes, uint32_t state,
                                  uint64_t max_samples) {
  return guarded(h, [&] {
    h->s->set_domain_maps(n_sizes ? std::vector<uint32_t>(sizes, sizes + n_sizes) : std::vector<uint32_t>(), state, max_samples);
  });
}
EPVD_API int epvd_reset_dmaps(epvd_sampler *h) {
  return guarded(h, [&] { h->s->reset_domain_maps(); });
}
EPVD_API int epvd_accumulate_dmaps(epvd_sampler *h) {
  return guarded(h, [&] { h->s->accumulate_domain_maps(); });
}
EPVD_API int epvd_dmaps_sizes(epvd_sampler *h, uint32_t *n_nodes, uint32_t *n_sizes, uint64_t *n_samples,
                                    uint64_t *n_sites) {
  return guarded(h, [&] {
    h->s->download_domain_maps(h->staged_dmaps_counts, h->staged_dmaps_edges, *n_nodes, *n_samples, *n_sites);
    *n_sizes = (uint32_t)h->s->domain_map_sizes().size();
    h->have_staged_dmaps = true;
  });
}
EPVD_API int epvd_download_dmaps(epvd_sampler *h, uint32_t *counts, uint64_t *edges) {
  return guarded(h, [&] {
    if (!h->have_staged_dmaps) throw std::runtime_error("epvd_dmaps_sizes first");
    std::copy(h->staged_dmaps_counts.begin(), h->staged_dmaps_counts.end(), counts);
    std::copy(h->staged_dmaps_edges.begin(), h->staged_dmaps_edges.end(), edges);
    h->staged_dmaps_counts.clear();
    h->staged_dmaps_edges.clear();
    h->have_staged_dmaps = false;
  });
}
EPVD_API int epvd_download_corr(epvd_sampler *h, uint32_t n_rows, uint32_t max_lag, uint64_t *n11, uint64_t *left1,
                                uint64_t *right1, uint64_t *n_samples) {
  return guarded(h, [&] {
    std::vector<uint64_t> a, l, r;
    uint32_t R = 0, L = 0;
    uint64_t ns = 0;
    h->s->download_spatial_correlation(a, l, r, R, L, ns);
    if (R != n_rows || L != max_lag)
      throw std::runtime_error("epvd_download_corr: n_rows must be the tree's nodes plus branches and max_lag the one set");
    std::copy(a.begin(), a.end(), n11);
    std::copy(l.begin(), l.end(), left1);
    std::copy(r.begin(), r.end(), right1);
    if (n_samples) *n_samples = ns;
  });
}

EPVD_API int epvd_set_epoch_stats(epvd_sampler *h, uint32_t P) {
  return guarded(h, [&] { h->s->set_epoch_stats(P); });
}
EPVD_API int epvd_epoch_stats_sizes(epvd_sampler *h, uint32_t *P, uint64_t *n_samples) {
  return guarded(h, [&] {
    uint64_t ns = 0;
    h->s->download_epoch_stats(h->staged_epoch, h->staged_epoch_k, h->staged_epoch_fixT, ns);
    h->have_staged_epoch = true;
    h->staged_epoch_ns = ns;
    *P = h->s->epoch_stats_epochs();
    *n_samples = ns;
  });
}
EPVD_API int epvd_download_epoch_stats(epvd_sampler *h, uint64_t *closed, int *k, uint64_t *fixT, double *J, double *D) {
  return guarded(h, [&] {
    if (!h->have_staged_epoch) throw std::runtime_error("epvd_epoch_stats_sizes first");
    if (closed) std::copy(h->staged_epoch.begin(), h->staged_epoch.end(), closed);
    if (k) std::copy(h->staged_epoch_k.begin() + 1, h->staged_epoch_k.end(), k);
    if (fixT) std::copy(h->staged_epoch_fixT.begin() + 1, h->staged_epoch_fixT.end(), fixT);
    if (J && D && h->staged_epoch_ns) {
      std::vector<double> j, d;
      h->s->epoch_counts_to_stats(h->staged_epoch, h->staged_epoch_k, h->staged_epoch_ns, j, d);
      std::copy(j.begin(), j.end(), J);
      std::copy(d.begin(), d.end(), D);
    }
    h->staged_epoch.clear();
    h->have_staged_epoch = false;
  });
}
