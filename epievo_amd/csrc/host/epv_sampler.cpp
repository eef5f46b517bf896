// epv_sampler.cpp -- see epv_sampler.hpp
#include "epv_sampler.hpp"
#include "epv_epochs.hpp"

#include <algorithm>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>

#include "epievo_mi355x.h"
#include "epv_domains.hpp"
#include "epv_turnover.hpp"
#include "epv_tracts.hpp"
#include "epv_corr.hpp"
#include "epv_dmaps.hpp"
#include "epievo_mi355x_comm.h"

namespace epv {

namespace {
const uint64_t kBlock = 256;   // sites per block: the unit of part cuts and halo widths
const uint32_t kMaxCap = 2047;   // EPV_MAX_CAP: 2 C + 1 segments must fit the 12-bit segment field of the Philox address

uint64_t round_to(double x, uint64_t unit) { return (uint64_t)(x / (double)unit + 0.5) * unit; }

// sites [lo, hi) of node-major flat paths
FlatPaths slice_sites(const FlatPaths &p, uint64_t lo, uint64_t hi) {
  FlatPaths q;
  q.n_sites = hi - lo;
  q.n_nodes = p.n_nodes;
  const uint64_t B = (uint64_t)p.n_nodes - 1, n = p.n_sites, m = hi - lo;
  q.init.resize(B * m);
  q.offsets.assign(B * m + 1, 0);
  for (uint64_t b = 0; b < B; ++b) {
    std::copy(p.init.begin() + b * n + lo, p.init.begin() + b * n + hi, q.init.begin() + b * m);
    const uint64_t j0 = p.offsets[b * n + lo], j1 = p.offsets[b * n + hi];
    for (uint64_t s = 0; s < m; ++s)
      q.offsets[b * m + s] = q.jumps.size() + (p.offsets[b * n + lo + s] - j0);
    q.jumps.insert(q.jumps.end(), p.jumps.begin() + j0, p.jumps.begin() + j1);
  }
  q.offsets[B * m] = q.jumps.size();
  return q;
}

// columns [lo, hi) of a genome of which `p` holds [first, first + p.n_sites): columns outside
// what is held come out blank (state 0, no jump) -- the halo columns of a slot whose neighbours
// live in other processes, filled by the first halo exchange
FlatPaths slice_sites_padded(const FlatPaths &p, uint64_t first, uint64_t lo, uint64_t hi) {
  if (lo >= first && hi <= first + p.n_sites) return slice_sites(p, lo - first, hi - first);
  const uint64_t a = std::max(lo, first), b = std::min(hi, first + p.n_sites);
  const FlatPaths mid = slice_sites(p, a - first, b - first);
  FlatPaths q;
  q.n_sites = hi - lo;
  q.n_nodes = p.n_nodes;
  const uint64_t B = (uint64_t)p.n_nodes - 1, m = hi - lo, mm = mid.n_sites, pad = a - lo;
  q.init.assign(B * m, 0);
  q.offsets.assign(B * m + 1, 0);
  q.jumps = mid.jumps;
  for (uint64_t br = 0; br < B; ++br) {
    std::copy(mid.init.begin() + br * mm, mid.init.begin() + (br + 1) * mm, q.init.begin() + br * m + pad);
    for (uint64_t s2 = 0; s2 < m; ++s2) {
      const uint64_t k = s2 < pad ? 0 : (s2 - pad < mm ? s2 - pad : mm);
      q.offsets[br * m + s2] = mid.offsets[br * mm + k];
    }
  }
  q.offsets[B * m] = mid.offsets[B * mm];
  return q;
}

FlatPaths concat_sites(const std::vector<FlatPaths> &parts) {
  FlatPaths q;
  q.n_nodes = parts[0].n_nodes;
  for (const FlatPaths &p : parts) q.n_sites += p.n_sites;
  const uint64_t B = (uint64_t)q.n_nodes - 1, n = q.n_sites;
  q.init.resize(B * n);
  q.offsets.assign(B * n + 1, 0);
  for (uint64_t b = 0; b < B; ++b) {
    uint64_t at = 0;
    for (const FlatPaths &p : parts) {
      const uint64_t m = p.n_sites;
      std::copy(p.init.begin() + b * m, p.init.begin() + (b + 1) * m, q.init.begin() + b * n + at);
      const uint64_t j0 = p.offsets[b * m], j1 = p.offsets[(b + 1) * m];
      for (uint64_t s = 0; s < m; ++s) q.offsets[b * n + at + s] = q.jumps.size() + (p.offsets[b * m + s] - j0);
      q.jumps.insert(q.jumps.end(), p.jumps.begin() + j0, p.jumps.begin() + j1);
      at += m;
    }
  }
  q.offsets[B * n] = q.jumps.size();
  return q;
}
}  // namespace

// One persistent host thread per part, started when a call first needs it and kept until the sampler goes:
// run(P, f) hands f(p) to worker p for p < P and returns when all of them are back -- what a spawn and a join
// of P fresh threads did on every run_mcmc, sweeps and download, without the thread start-up between the end of
// one E-step and the first launch of the next.  A part stays with its thread (a HIP thread keeps its device).
// An exception that leaves f(p) is carried over and rethrown by run (the first by part index) after every
// worker has finished; if a thread cannot be started, run throws before any work was handed out.
class SingleSiteSampler::Workers {
public:
  ~Workers() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    work_.notify_all();
    for (std::thread &t : th_) t.join();
  }
  void run(size_t P, const std::function<void(size_t)> &f) {
    if (P == 0) return;
    std::unique_lock<std::mutex> lk(m_);
    while (th_.size() < P) {
      const size_t i = th_.size();
      const uint64_t g0 = gen_;
      th_.emplace_back([this, i, g0] { loop(i, g0); });
    }
    errs_.assign(P, nullptr);
    f_ = &f;
    n_ = P;
    pending_ = P;
    ++gen_;
    work_.notify_all();
    done_.wait(lk, [this] { return pending_ == 0; });
    f_ = nullptr;
    n_ = 0;
    for (std::exception_ptr &e : errs_)
      if (e) std::rethrow_exception(e);
  }

private:
  void loop(size_t i, uint64_t seen) {
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      work_.wait(lk, [&] { return stop_ || (gen_ != seen && i < n_); });
      if (stop_) return;
      seen = gen_;
      const std::function<void(size_t)> *f = f_;
      lk.unlock();
      std::exception_ptr e;
      try {
        (*f)(i);
      } catch (...) {
        e = std::current_exception();
      }
      lk.lock();
      errs_[i] = e;
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::mutex m_;
  std::condition_variable work_, done_;
  std::vector<std::thread> th_;
  std::vector<std::exception_ptr> errs_;
  const std::function<void(size_t)> *f_ = nullptr;
  size_t n_ = 0, pending_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

void SingleSiteSampler::on_parts(const std::function<void(size_t)> &f) {
  if (!workers_) workers_.reset(new Workers());
  workers_->run(parts_.size(), f);
}

std::vector<int> parse_device_list(const std::string &spec) {
  std::vector<int> out;
  if (spec.empty()) return {0};
  if (spec == "all") {
    // every GPU HIP shows; counted by probing contexts so that this file needs no HIP header
    for (int d = 0; d < 64; ++d) {
      epv_ctx *c = epv_create(d);
      if (!c) break;
      epv_destroy(c);
      out.push_back(d);
    }
    if (out.empty()) throw std::runtime_error("no HIP device found (this build has no CPU fallback)");
    return out;
  }
  std::stringstream ss(spec);
  std::string tok;
  while (std::getline(ss, tok, ',')) {
    char *end = nullptr;
    const long v = std::strtol(tok.c_str(), &end, 10);
    if (tok.empty() || *end != '\0' || v < 0) throw std::runtime_error("bad device list: " + spec);
    out.push_back((int)v);
  }
  if (out.empty()) throw std::runtime_error("bad device list: " + spec);
  return out;
}

std::vector<int> devices_from_env() {
  const char *e = std::getenv("EPV_DEVICES");
  return parse_device_list(e ? e : "");
}

SingleSiteSampler::SingleSiteSampler(size_t n_burn_in, size_t n_batch, int device, uint32_t capacity)
    : SingleSiteSampler(n_burn_in, n_batch, std::vector<int>(1, device), capacity) {}

SingleSiteSampler::SingleSiteSampler(size_t n_burn_in, size_t n_batch, const std::vector<int> &devices,
                                     uint32_t capacity)
    : SAMPLE_ROOT(false), burn_in(n_burn_in), batch(n_batch), ctx_(nullptr), devices_(devices),
      capacity_(capacity) {
  if (devices_.empty()) devices_.push_back(0);
  ctx_ = epv_create(devices_[0]);
  if (!ctx_)
    throw std::runtime_error("cannot open HIP device " + std::to_string(devices_[0]) +
                             " (this build has no CPU fallback)");
  if (const char *e = std::getenv("EPV_CONTEXTS_PER_GPU")) contexts_wanted_ = std::max(1, std::atoi(e));
  if (const char *e = std::getenv("EPV_ROW_BLOCKS")) {
    const int v = std::atoi(e);
    if (v < 1 || v > 4096 || (v & (v - 1))) throw std::runtime_error("EPV_ROW_BLOCKS must be a power of two");
    row_blocks_ = (uint32_t)v;
  }
  if (const char *e = std::getenv("EPV_FORCE_COMM")) force_comm_ = std::atoi(e) != 0;
}

SingleSiteSampler::SingleSiteSampler(size_t n_burn_in, size_t n_batch, const RankSpec &rank, uint32_t capacity)
    : SingleSiteSampler(n_burn_in, n_batch, std::vector<int>(1, rank.device), capacity) {
  if (rank.world < 1 || rank.rank < 0 || rank.rank >= rank.world) throw std::runtime_error("bad rank / world");
  rank_mode_ = true;
  rank_ = rank;
  world_ = (size_t)rank.world;
}

SingleSiteSampler::~SingleSiteSampler() {
  drop_parts();
  if (rank_comm_) epv_comm_destroy(rank_comm_);
  epv_destroy(ctx_);
}

std::vector<epv_ctx *> SingleSiteSampler::contexts() const {
  std::vector<epv_ctx *> v;
  if (parts_.empty()) v.push_back(ctx_);
  for (const Part &p : parts_) v.push_back(p.ctx);
  return v;
}
void SingleSiteSampler::set_options(uint32_t flags) {
  SAMPLE_ROOT = (flags & (uint32_t)EPV_OPT_SAMPLE_ROOT) != 0;
  for (epv_ctx *c : contexts()) check_on(c, epv_set_options(c, flags), "epv_set_options");
  options_ = flags;
}
void SingleSiteSampler::set_timing(int every) {
  for (epv_ctx *c : contexts()) check_on(c, epv_set_timing(c, every), "epv_set_timing");
}
void SingleSiteSampler::kernel_time_ms(double &avg_ms, uint64_t &n_launches) {
  double tot = 0.0;
  n_launches = 0;
  for (epv_ctx *c : contexts()) {
    double a = 0.0;
    uint64_t k = 0;
    check_on(c, epv_kernel_time_ms(c, &a, &k), "epv_kernel_time_ms");
    tot += a * (double)k;
    n_launches += k;
  }
  avg_ms = n_launches ? tot / (double)n_launches : 0.0;
}
uint32_t SingleSiteSampler::phase_mode() {
  uint32_t m = 0;
  epv_ctx *c = contexts()[0];
  check_on(c, epv_phase_mode(c, &m), "epv_phase_mode");
  return m;
}

void SingleSiteSampler::free_stat_buffers() {
  for (Slot &s : slots_) {
    epv_ctx *c = parts_[s.part0].ctx;
    if (s.d_piece) epv_dev_free(c, s.d_piece);
    if (s.d_gather) epv_dev_free(c, s.d_gather);
    s.d_piece = s.d_gather = nullptr;
  }
  stat_batch_ = 0;
}

void SingleSiteSampler::drop_parts() {
  free_stat_buffers();
  for (Slot &s : slots_) {
    epv_ctx *c = parts_[s.part0].ctx;
    for (void *&p : s.d_halo) { if (p) epv_dev_free(c, p); p = nullptr; }
    if (s.comm && s.comm != rank_comm_) epv_comm_destroy(s.comm);
    s.comm = nullptr;
  }
  for (Part &p : parts_) if (p.ctx != ctx_) epv_destroy(p.ctx);
  parts_.clear();
  slots_.clear();
}

bool SingleSiteSampler::uses_rccl() const {
  return !slots_.empty() && slots_[0].comm && epv_comm_is_rccl(slots_[0].comm);
}

std::string SingleSiteSampler::layout() const {
  std::ostringstream o;
  if (!sharded()) { o << "1 context on device " << devices_[0]; return o.str(); }
  o << world_ << " GPU slot(s)";
  if (rank_mode_) o << " (this process: slot " << rank_.rank << ")";
  o << " x up to " << contexts_per_gpu() << " context(s) = " << parts_.size() << " parts"
    << (rank_mode_ ? " here" : "") << ", halo " << halo_ << " columns";
  if (slots_[0].comm) o << ", exchange over " << (uses_rccl() ? "RCCL" : "the loopback transport");
  o << "; devices";
  for (const Slot &s : slots_) o << " " << s.device;
  return o.str();
}

void SingleSiteSampler::check_on(epv_ctx *c, int rc, const char *what) {
  if (rc != EPV_OK) throw std::runtime_error(std::string(what) + ": " + epv_last_error(c));
}
void SingleSiteSampler::check_comm(epv_comm *c, int rc, const char *what) {
  if (rc != EPV_OK) throw std::runtime_error(std::string(what) + ": " + epv_comm_last_error(c));
}
void SingleSiteSampler::check(int rc, const char *what) { check_on(ctx_, rc, what); }

// after an MCMC call: an overflow leaves a valid chain and complete outputs (the over-long
// proposals were rejected), so widen the jump slots for the following calls -- what the
// reference's std::vector paths do on their own -- and carry on
void SingleSiteSampler::check_mcmc(int rc, const char *what) {
  if (rc == EPV_ERR_CAPACITY) {
    uint32_t cap = 0;
    if (epv_get_capacity(ctx_, &cap) == EPV_OK && cap < kMaxCap) {
      const std::string msg = epv_last_error(ctx_);
      check(epv_set_capacity(ctx_, std::min(kMaxCap, cap * 2u)), "epv_set_capacity");
      capacity_events.push_back(std::string(what) + ": " + msg);
      return;
    }
  }
  check(rc, what);
}

void SingleSiteSampler::equalize_capacity() {
  uint32_t cap = 0;
  for (Part &p : parts_) { uint32_t v = 0; check_on(p.ctx, epv_get_capacity(p.ctx, &v), "epv_get_capacity"); cap = std::max(cap, v); }
  for (Part &p : parts_) check_on(p.ctx, epv_set_capacity(p.ctx, cap), "epv_set_capacity");
}

// Before every reset of a sharded genome: equal jump-slot widths (an overflow may have widened
// one part), each part's edge columns into its neighbour's halo -- a device-to-device copy
// inside a GPU, one RCCL send/receive pair per GPU boundary -- and the halos marked fresh.
void SingleSiteSampler::refresh_parts() {
  const size_t P = parts_.size();
  const uint64_t H = halo_;
  equalize_capacity();
  const uint64_t bytes = H * epv_column_bytes(parts_[0].ctx);
  // between two parts of one GPU: device-to-device copies
  for (size_t p = 0; p + 1 < P; ++p) {
    Part &L = parts_[p], &R = parts_[p + 1];
    if (L.slot != R.slot) continue;
    // (no host wait: the unpack sits on the receiving context's stream, in front of its reset;
    // a part's right-going edge uses half 0 of its staging buffer, its left-going edge half 1)
    check_on(R.ctx, epv_copy_columns_async(L.ctx, L.b - H - L.lo, H, R.ctx, 0, 0), "epv_copy_columns_async");
    check_on(L.ctx, epv_copy_columns_async(R.ctx, H, H, L.ctx, L.b - L.lo, 1), "epv_copy_columns_async");
  }
  // between two GPU slots: the first part of a slot sends its left edge to the slot before it, the
  // last part its right edge to the slot after it -- one exchange call per slot that lives here
  // (all of them, or this process's one), the neighbours' calls pair up inside RCCL
  if (world_ > 1) {
    for (Slot &s : slots_) {
      epv_ctx *c = parts_[s.part0].ctx;
      if (s.halo_bytes != bytes) {
        for (void *&q : s.d_halo) {
          if (q) check_on(c, epv_dev_free(c, q), "epv_dev_free");
          q = nullptr;
          check_on(c, epv_dev_alloc(c, bytes, &q), "epv_dev_alloc");
        }
        s.halo_bytes = bytes;
      }
      Part &F = parts_[s.part0], &Lp = parts_[s.part1 - 1];
      if (s.gidx > 0) check_on(F.ctx, epv_pack_columns_dev(F.ctx, F.a - F.lo, H, s.d_halo[0]), "epv_pack_columns_dev");
      if (s.gidx + 1 < world_)
        check_on(Lp.ctx, epv_pack_columns_dev(Lp.ctx, Lp.b - H - Lp.lo, H, s.d_halo[2]), "epv_pack_columns_dev");
    }
    if (epv_comm_group_start() != EPV_OK) throw std::runtime_error("epv_comm_group_start failed");
    for (Slot &s : slots_)
      check_comm(s.comm, epv_comm_exchange(s.comm, s.d_halo[0], s.d_halo[1], s.gidx > 0 ? bytes : 0, s.d_halo[2],
                                           s.d_halo[3], s.gidx + 1 < world_ ? bytes : 0), "epv_comm_exchange");
    if (epv_comm_group_end() != EPV_OK) throw std::runtime_error("epv_comm_group_end failed (halo exchange)");
    for (Slot &s : slots_) check_comm(s.comm, epv_comm_sync(s.comm), "epv_comm_sync");
    for (Slot &s : slots_) {
      Part &F = parts_[s.part0], &Lp = parts_[s.part1 - 1];
      if (s.gidx > 0) check_on(F.ctx, epv_unpack_columns_dev(F.ctx, 0, H, s.d_halo[1]), "epv_unpack_columns_dev");
      if (s.gidx + 1 < world_)
        check_on(Lp.ctx, epv_unpack_columns_dev(Lp.ctx, Lp.b - Lp.lo, H, s.d_halo[3]), "epv_unpack_columns_dev");
    }
  }
  for (size_t p = 0; p < P; ++p) {
    const bool first = parts_[p].lo == parts_[p].a, last = parts_[p].hi == parts_[p].b;   // the genome's ends
    check_on(parts_[p].ctx, epv_set_halo(parts_[p].ctx, first ? 0 : H, last ? 0 : H), "epv_set_halo");
  }
}

// SAMPLE_ROOT (a public field of the reference class, hard-wired false at SingleSiteSampler.cpp:441 and
// set by none of its programs): the proposal also draws the root state (:167-176, :246-249).  The
// field is forwarded to every context as EPV_OPT_SAMPLE_ROOT before each call that runs updates, together
// with the other options of set_options: every context runs with the same word.
void SingleSiteSampler::apply_sample_root() {
  const uint32_t bit = (uint32_t)EPV_OPT_SAMPLE_ROOT;
  options_ = SAMPLE_ROOT ? (options_ | bit) : (options_ & ~bit);
  for (epv_ctx *c : contexts()) {
    uint32_t flags = 0;
    check_on(c, epv_get_options(c, &flags), "epv_get_options");
    if (flags != options_) check_on(c, epv_set_options(c, options_), "epv_set_options");
  }
}

// a halo that lasts one whole run_mcmc (two columns per colour phase), in whole blocks
static uint64_t halo_for(size_t n_burn_in, size_t n_batch) {
  return std::max<uint64_t>(kBlock, (6 * (uint64_t)(n_burn_in + n_batch) + 2 + kBlock - 1) / kBlock * kBlock);
}

std::vector<uint64_t> SingleSiteSampler::shard_cuts(uint64_t n, size_t world, size_t n_burn_in, size_t n_batch,
                                                    uint32_t row_blocks) {
  const uint64_t H = halo_for(n_burn_in, n_batch);
  const uint64_t min_part = 2 * H + 2 * kBlock;     // every part must own more than its halos
  const uint64_t RS = kBlock * row_blocks;
  size_t G = std::max<size_t>(1, world);
  std::vector<uint64_t> cut;
  for (;; --G) {
    cut.assign(G + 1, 0);
    cut[G] = n;
    bool ok = true;
    for (size_t g = 1; g < G; ++g) cut[g] = round_to((double)g * (double)n / (double)G, RS);
    for (size_t g = 0; g < G && ok; ++g) ok = cut[g + 1] > cut[g] && cut[g + 1] - cut[g] >= min_part;
    if (ok || G == 1) break;
  }
  return cut;
}

void SingleSiteSampler::reset(const Model &m, const Tree &th, const FlatPaths &paths) {
  if (rank_mode_) throw std::runtime_error("one slot per process: reset(model, tree, owned columns, n_global)");
  build(th, paths, paths.n_sites, false);
  reset(m);
  if (pa_points_) set_path_average(pa_points_);
  if (bevents_) set_branch_events(true);
  if (wstat_W_) set_window_stats(wstat_W_);
  if (epoch_P_) set_epoch_stats(epoch_P_);
  if (origins_) set_lineage_origins(true);
  if (domains_max_) set_domain_stats(domains_max_);
  if (patterns_) set_change_patterns(true);
  if (turnover_max_) set_domain_turnover(turnover_max_);
  if (corr_lag_) set_spatial_correlation(corr_lag_, corr_max_);
  if (mixing_lag_) enable_mixing(mixing_lag_);
  if (!dmaps_sizes_.empty()) set_domain_maps(dmaps_sizes_, dmaps_state_, dmaps_max_);
  if (tracts_max_) set_change_tracts(tracts_max_);
}

void SingleSiteSampler::reset(const Model &m, const Tree &th, const FlatPaths &owned, uint64_t n_global) {
  if (!rank_mode_) throw std::runtime_error("reset(..., n_global) belongs to the one-slot-per-process constructor");
  build(th, owned, n_global, true);
  reset(m);
  if (pa_points_) set_path_average(pa_points_);
  if (bevents_) set_branch_events(true);
  if (wstat_W_) set_window_stats(wstat_W_);
  if (epoch_P_) set_epoch_stats(epoch_P_);
  if (origins_) set_lineage_origins(true);
  if (domains_max_) set_domain_stats(domains_max_);
  if (patterns_) set_change_patterns(true);
  if (turnover_max_) set_domain_turnover(turnover_max_);
  if (corr_lag_) set_spatial_correlation(corr_lag_, corr_max_);
  if (mixing_lag_) enable_mixing(mixing_lag_);
  if (!dmaps_sizes_.empty()) set_domain_maps(dmaps_sizes_, dmaps_state_, dmaps_max_);
  if (tracts_max_) set_change_tracts(tracts_max_);
}

void SingleSiteSampler::set_path_average(uint32_t n_points) {
  // before the first reset(model, tree, paths) there are no paths to lay the counts out for: the
  // setting is applied to the contexts that reset builds
  if (n_sites_ || n_points == 0)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_path_average(c, n_points), "epv_set_path_average");
  pa_points_ = n_points;
}

void SingleSiteSampler::download_path_average(std::vector<uint32_t> &counts, uint64_t &n_samples) {
  if (!pa_points_) throw std::runtime_error("path average is off: set_path_average first");
  const std::vector<epv_ctx *> cs = contexts();
  const uint64_t B = (uint64_t)n_nodes_ - 1u, P = pa_points_;
  std::vector<uint64_t> first(cs.size()), count(cs.size());
  uint64_t total = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint32_t p = 0;
    check_on(cs[i], epv_path_average_layout(cs[i], &p, &first[i], &count[i]), "epv_path_average_layout");
    if (p != P) throw std::runtime_error("a context's path average is off");
    uint64_t ns = 0;
    check_on(cs[i], epv_path_average_samples(cs[i], &ns), "epv_path_average_samples");
    if (i == 0) n_samples = ns;
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of path-average samples");
    total += count[i];
  }
  counts.assign(B * total * P, 0u);
  std::vector<uint32_t> part;
  uint64_t at = 0;
  for (size_t i = 0; i < cs.size(); ++i) {   // contexts in genome order, each one's sites contiguous
    part.assign(B * count[i] * P, 0u);
    if (count[i]) check_on(cs[i], epv_get_path_average(cs[i], first[i], count[i], part.data()), "epv_get_path_average");
    for (uint64_t b = 0; b < B; ++b)
      std::copy(part.begin() + b * count[i] * P, part.begin() + (b + 1) * count[i] * P,
                counts.begin() + (b * total + at) * P);
    at += count[i];
  }
}

void SingleSiteSampler::set_branch_events(bool on) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || !on)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_branch_events(c, on ? 1 : 0), "epv_set_branch_events");
  bevents_ = on;
}

static uint64_t branch_event_samples(const std::vector<epv_ctx *> &cs) {
  uint64_t n_samples = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint64_t ns = 0;
    if (epv_branch_events_samples(cs[i], &ns) != EPV_OK) throw std::runtime_error("epv_branch_events_samples failed");
    if (i == 0) n_samples = ns;
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of branch-event samples");
  }
  return n_samples;
}

void SingleSiteSampler::download_branch_events(std::vector<uint32_t> &planes, uint64_t &n_samples) {
  if (!bevents_) throw std::runtime_error("branch events are off: set_branch_events first");
  const std::vector<epv_ctx *> cs = contexts();
  const uint64_t R = 6u * ((uint64_t)n_nodes_ - 1u);
  std::vector<uint64_t> first(cs.size()), count(cs.size());
  uint64_t total = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    check_on(cs[i], epv_branch_events_layout(cs[i], &first[i], &count[i]), "epv_branch_events_layout");
    total += count[i];
  }
  n_samples = branch_event_samples(cs);
  planes.assign(R * total, 0u);
  std::vector<uint32_t> part;
  uint64_t at = 0;
  for (size_t i = 0; i < cs.size(); ++i) {   // contexts in genome order, each one's sites contiguous
    part.assign(R * count[i], 0u);
    if (count[i]) check_on(cs[i], epv_get_branch_events(cs[i], first[i], count[i], part.data()), "epv_get_branch_events");
    for (uint64_t r = 0; r < R; ++r)
      std::copy(part.begin() + r * count[i], part.begin() + (r + 1) * count[i], planes.begin() + r * total + at);
    at += count[i];
  }
}

void SingleSiteSampler::download_branch_event_windows(uint64_t W, std::vector<uint64_t> &sums, uint64_t &n_samples) {
  if (!bevents_) throw std::runtime_error("branch events are off: set_branch_events first");
  if (W == 0) throw std::runtime_error("a window holds at least one site");
  const std::vector<epv_ctx *> cs = contexts();
  const uint64_t R = 6u * ((uint64_t)n_nodes_ - 1u), nw = (n_sites_ + W - 1u) / W;
  n_samples = branch_event_samples(cs);
  sums.assign(R * nw, 0u);
  std::vector<uint64_t> part(R * nw);
  for (epv_ctx *c : cs) {   // every context's contribution to the windows of global sites
    check_on(c, epv_get_branch_event_windows(c, W, 0u, nw, part.data()), "epv_get_branch_event_windows");
    for (size_t k = 0; k < part.size(); ++k) sums[k] += part[k];
  }
}

void SingleSiteSampler::enable_mixing(uint32_t max_lag) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (max_lag > 16u) throw std::runtime_error("max_lag of the mixing diagnostics: 1 .. 16 (0 turns them off)");
  if (n_sites_ || !max_lag)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_mixing(c, max_lag), "epv_set_mixing");
  mixing_lag_ = max_lag;
}

// samples, moved_pairs, pairs[1 .. K]: the contexts ran the same runs
static void mixing_words(const std::vector<epv_ctx *> &cs, uint32_t K, std::vector<uint64_t> &words) {
  std::vector<uint64_t> w(K + 2u);
  for (size_t i = 0; i < cs.size(); ++i) {
    if (epv_mixing_pairs(cs[i], w.data()) != EPV_OK) throw std::runtime_error(std::string("epv_mixing_pairs: ") + epv_last_error(cs[i]));
    if (i == 0) words = w;
    else if (w[0] != words[0]) throw std::runtime_error("the contexts hold different numbers of mixing samples");
    else if (w != words) throw std::runtime_error("the contexts hold mixing samples of different runs (their pair counts differ)");
  }
}

void SingleSiteSampler::download_mixing(std::vector<uint64_t> &words, std::vector<uint32_t> &moved,
                                        std::vector<uint64_t> &sums) {
  if (!mixing_lag_) throw std::runtime_error("mixing diagnostics are off: enable_mixing first");
  const std::vector<epv_ctx *> cs = contexts();
  const uint64_t R = 2u + mixing_lag_;
  std::vector<uint64_t> first(cs.size()), count(cs.size());
  uint64_t total = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint32_t K = 0;
    check_on(cs[i], epv_mixing_layout(cs[i], &first[i], &count[i], &K), "epv_mixing_layout");
    if (K != mixing_lag_) throw std::runtime_error("a context's mixing diagnostics are off");
    total += count[i];
  }
  mixing_words(cs, mixing_lag_, words);
  moved.assign(total, 0u);
  sums.assign(R * total, 0u);
  std::vector<uint64_t> part;
  uint64_t at = 0;
  for (size_t i = 0; i < cs.size(); ++i) {   // contexts in genome order, each one's sites contiguous
    part.assign(R * count[i], 0u);
    if (count[i])
      check_on(cs[i], epv_mixing_counts(cs[i], first[i], count[i], moved.data() + at, part.data()), "epv_mixing_counts");
    for (uint64_t r = 0; r < R; ++r)
      std::copy(part.begin() + r * count[i], part.begin() + (r + 1) * count[i], sums.begin() + r * total + at);
    at += count[i];
  }
}

void SingleSiteSampler::set_change_patterns(bool on) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || !on)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_change_patterns(c, on ? 1 : 0), "epv_set_change_patterns");
  patterns_ = on;
}

// the sample count and the row count, the same on every context; first and count per context when asked for
void SingleSiteSampler::change_pattern_layouts(const std::vector<epv_ctx *> &cs, uint32_t &n_rows, uint64_t &n_samples,
                                               std::vector<uint64_t> *first, std::vector<uint64_t> *count) {
  n_rows = 0;
  n_samples = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint32_t R = 0, I = 0;
    uint64_t a = 0, k = 0, ns = 0;
    check_on(cs[i], epv_change_patterns_layout(cs[i], &R, &I, nullptr, &a, &k), "epv_change_patterns_layout");
    check_on(cs[i], epv_change_patterns_samples(cs[i], &ns), "epv_change_patterns_samples");
    if (i == 0) { n_rows = R; n_samples = ns; }
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of change-pattern samples");
    else if (R != n_rows) throw std::runtime_error("the contexts hold different numbers of change-pattern rows");
    if (first) (*first)[i] = a;
    if (count) (*count)[i] = k;
  }
}

void SingleSiteSampler::download_change_patterns(std::vector<uint32_t> &rows, uint32_t &n_rows, uint64_t &n_samples) {
  if (!patterns_) throw std::runtime_error("change patterns are off: set_change_patterns first");
  const std::vector<epv_ctx *> cs = contexts();
  std::vector<uint64_t> first(cs.size()), count(cs.size());
  change_pattern_layouts(cs, n_rows, n_samples, &first, &count);
  const uint64_t R = n_rows;
  uint64_t total = 0;
  for (uint64_t k : count) total += k;
  rows.assign(R * total, 0u);
  std::vector<uint32_t> part;
  uint64_t at = 0;
  for (size_t i = 0; i < cs.size(); ++i) {   // contexts in genome order, each one's sites contiguous
    part.assign(R * count[i], 0u);
    if (count[i]) check_on(cs[i], epv_get_change_patterns(cs[i], first[i], count[i], part.data()), "epv_get_change_patterns");
    for (uint64_t r = 0; r < R; ++r)
      std::copy(part.begin() + r * count[i], part.begin() + (r + 1) * count[i], rows.begin() + r * total + at);
    at += count[i];
  }
}

void SingleSiteSampler::download_change_pattern_windows(uint64_t W, std::vector<uint64_t> &sums, uint32_t &n_rows,
                                                        uint64_t &n_samples) {
  if (!patterns_) throw std::runtime_error("change patterns are off: set_change_patterns first");
  if (W == 0) throw std::runtime_error("a window holds at least one site");
  const std::vector<epv_ctx *> cs = contexts();
  change_pattern_layouts(cs, n_rows, n_samples, nullptr, nullptr);
  const uint64_t nw = (n_sites_ + W - 1u) / W;
  sums.assign((uint64_t)n_rows * nw, 0u);
  std::vector<uint64_t> part(sums.size());
  for (epv_ctx *c : cs) {   // every context's contribution to the windows of global sites
    check_on(c, epv_get_change_pattern_windows(c, W, 0u, nw, part.data()), "epv_get_change_pattern_windows");
    for (size_t k = 0; k < part.size(); ++k) sums[k] += part[k];
  }
}

void SingleSiteSampler::set_window_stats(uint64_t W) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || !W)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_window_stats(c, W), "epv_set_window_stats");
  wstat_W_ = W;
}

void SingleSiteSampler::download_window_stats(std::vector<int64_t> &counts, uint64_t &W, uint64_t &n_windows,
                                              uint64_t &n_samples) {
  if (!wstat_W_) throw std::runtime_error("window statistics are off: set_window_stats first");
  const std::vector<epv_ctx *> cs = contexts();
  W = window_stats_width();
  n_windows = window_stats_windows();
  n_samples = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint64_t ns = 0;
    if (epv_window_stats_samples(cs[i], &ns) != EPV_OK) throw std::runtime_error("epv_window_stats_samples failed");
    if (i == 0) n_samples = ns;
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of window-statistics samples");
  }
  const uint64_t V = 16u * ((uint64_t)n_nodes_ - 1u);
  counts.assign(V * n_windows, 0);
  std::vector<int64_t> part(V * n_windows);
  for (epv_ctx *c : cs) {   // every context's contribution to the windows of global sites, as integers
    check_on(c, epv_get_window_stats(c, 0u, n_windows, part.data()), "epv_get_window_stats");
    for (size_t k = 0; k < part.size(); ++k) counts[k] += part[k];
  }
}

void SingleSiteSampler::window_counts_to_stats(const std::vector<int64_t> &counts, uint64_t n_windows, uint64_t n_samples,
                                               std::vector<double> &J, std::vector<double> &D) {
  const uint64_t B = (uint64_t)n_nodes_ - 1u;
  if (counts.size() != n_windows * B * 16u) throw std::runtime_error("window_counts_to_stats: counts of the wrong size");
  J.assign(n_windows * B * 8u, 0.0);
  D.assign(n_windows * B * 8u, 0.0);
  epv_ctx *c = contexts().at(0);
  if (n_windows)
    check_on(c, epv_window_counts_to_stats(c, counts.data(), n_windows, n_samples, J.data(), D.data()),
             "epv_window_counts_to_stats");
}

std::vector<int> SingleSiteSampler::window_stats_scale_exps() {
  if (!wstat_W_) throw std::runtime_error("window statistics are off: set_window_stats first");
  std::vector<int> k((size_t)n_nodes_, 0);
  epv_ctx *c = contexts().at(0);     // (every context of a genome has its tree and its n_global)
  if (n_nodes_ > 1) check_on(c, epv_window_stats_scale_exps(c, k.data() + 1), "epv_window_stats_scale_exps");
  return k;
}

void SingleSiteSampler::set_lineage_origins(bool on) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || !on)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_lineage_origins(c, on ? 1 : 0), "epv_set_lineage_origins");
  origins_ = on;
}

void SingleSiteSampler::reset_lineage_origins() {
  if (!origins_) throw std::runtime_error("lineage origins are off: set_lineage_origins first");
  for (epv_ctx *c : contexts()) check_on(c, epv_reset_lineage_origins(c), "epv_reset_lineage_origins");
}

void SingleSiteSampler::accumulate_lineage_origins() {
  if (!origins_) throw std::runtime_error("lineage origins are off: set_lineage_origins first");
  for (epv_ctx *c : contexts()) check_on(c, epv_accumulate_lineage_origins(c), "epv_accumulate_lineage_origins");
}

// the sample count and the scale exponent every context agrees on
static uint64_t lineage_origin_samples(const std::vector<epv_ctx *> &cs, int &k) {
  uint64_t n_samples = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint64_t ns = 0;
    int ki = 0;
    if (epv_lineage_origins_samples(cs[i], &ns) != EPV_OK) throw std::runtime_error("epv_lineage_origins_samples failed");
    if (epv_lineage_origins_scale_exp(cs[i], &ki) != EPV_OK)
      throw std::runtime_error(std::string("epv_lineage_origins_scale_exp: ") + epv_last_error(cs[i]));
    if (i == 0) { n_samples = ns; k = ki; }
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of lineage-origin samples");
    else if (ki != k) throw std::runtime_error("the contexts hold lineage-origin ages of different scales");
  }
  return n_samples;
}

void SingleSiteSampler::lineage_origin_rows(std::vector<uint32_t> &leaf_node, std::vector<uint32_t> &branch_node) {
  if (!origins_) throw std::runtime_error("lineage origins are off: set_lineage_origins first");
  epv_ctx *c = contexts().at(0);     // (every context of a genome has its tree)
  uint32_t L = 0, R = 0;
  uint64_t first = 0, count = 0;
  check_on(c, epv_lineage_origins_layout(c, &L, &R, &first, &count), "epv_lineage_origins_layout");
  leaf_node.assign(R, 0u);
  branch_node.assign(R, 0u);
  if (R) check_on(c, epv_lineage_origin_rows(c, leaf_node.data(), branch_node.data()), "epv_lineage_origin_rows");
}

int SingleSiteSampler::lineage_origins_scale_exp() {
  if (!origins_) throw std::runtime_error("lineage origins are off: set_lineage_origins first");
  int k = 0;
  (void)lineage_origin_samples(contexts(), k);
  return k;
}

void SingleSiteSampler::download_lineage_origins(std::vector<uint32_t> &origin, std::vector<uint64_t> &age, int &k,
                                                 uint64_t &n_samples) {
  if (!origins_) throw std::runtime_error("lineage origins are off: set_lineage_origins first");
  const std::vector<epv_ctx *> cs = contexts();
  std::vector<uint64_t> first(cs.size()), count(cs.size());
  uint64_t total = 0;
  uint32_t L = 0, R = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    check_on(cs[i], epv_lineage_origins_layout(cs[i], &L, &R, &first[i], &count[i]), "epv_lineage_origins_layout");
    total += count[i];
  }
  n_samples = lineage_origin_samples(cs, k);
  origin.assign((uint64_t)R * total, 0u);
  age.assign((uint64_t)L * total, 0u);
  std::vector<uint32_t> po;
  std::vector<uint64_t> pa;
  uint64_t at = 0;
  for (size_t i = 0; i < cs.size(); ++i) {   // contexts in genome order, each one's sites contiguous
    po.assign((uint64_t)R * count[i], 0u);
    pa.assign((uint64_t)L * count[i], 0u);
    if (count[i])
      check_on(cs[i], epv_get_lineage_origins(cs[i], first[i], count[i], po.data(), pa.data()), "epv_get_lineage_origins");
    for (uint64_t r = 0; r < R; ++r)
      std::copy(po.begin() + r * count[i], po.begin() + (r + 1) * count[i], origin.begin() + r * total + at);
    for (uint64_t l = 0; l < L; ++l)
      std::copy(pa.begin() + l * count[i], pa.begin() + (l + 1) * count[i], age.begin() + l * total + at);
    at += count[i];
  }
}

void SingleSiteSampler::download_lineage_origin_windows(uint64_t W, std::vector<uint64_t> &origin,
                                                        std::vector<uint64_t> &age, int &k, uint64_t &n_samples) {
  if (!origins_) throw std::runtime_error("lineage origins are off: set_lineage_origins first");
  if (W == 0) throw std::runtime_error("a window holds at least one site");
  const std::vector<epv_ctx *> cs = contexts();
  uint32_t L = 0, R = 0;
  uint64_t first = 0, count = 0;
  check_on(cs.at(0), epv_lineage_origins_layout(cs[0], &L, &R, &first, &count), "epv_lineage_origins_layout");
  const uint64_t nw = (n_sites_ + W - 1u) / W;
  n_samples = lineage_origin_samples(cs, k);
  std::vector<uint64_t> sums(((uint64_t)R + L) * nw, 0u), part(((uint64_t)R + L) * nw);
  for (epv_ctx *c : cs) {   // every context's contribution to the windows of global sites
    check_on(c, epv_get_lineage_origin_windows(c, W, 0u, nw, part.data()), "epv_get_lineage_origin_windows");
    for (size_t i = 0; i < part.size(); ++i) {
      if (part[i] > UINT64_MAX - sums[i])   // (a context alone refuses such a sum: so does their total)
        throw std::runtime_error("the age sum of a window passes 64 bits: use narrower windows");
      sums[i] += part[i];
    }
  }
  origin.assign(sums.begin(), sums.begin() + (uint64_t)R * nw);
  age.assign(sums.begin() + (uint64_t)R * nw, sums.end());
}

void SingleSiteSampler::set_domain_stats(uint64_t max_samples) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || !max_samples)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_domain_stats(c, max_samples), "epv_set_domain_stats");
  domains_max_ = max_samples;
}

void SingleSiteSampler::reset_domain_stats() {
  if (!domains_max_) throw std::runtime_error("domain statistics are off: set_domain_stats first");
  for (epv_ctx *c : contexts()) check_on(c, epv_reset_domain_stats(c), "epv_reset_domain_stats");
}

void SingleSiteSampler::accumulate_domain_stats() {
  if (!domains_max_) throw std::runtime_error("domain statistics are off: set_domain_stats first");
  for (epv_ctx *c : contexts()) check_on(c, epv_accumulate_domain_stats(c), "epv_accumulate_domain_stats");
}

void SingleSiteSampler::download_domain_part(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum,
                                             std::vector<uint64_t> &edges, uint32_t &n_nodes, uint64_t &n_samples) {
  if (!domains_max_) throw std::runtime_error("domain statistics are off: set_domain_stats first");
  const std::vector<epv_ctx *> cs = contexts();   // in genome order
  std::vector<std::vector<uint64_t>> h(cs.size()), l(cs.size()), e(cs.size());
  std::vector<const uint64_t *> hp(cs.size()), lp(cs.size()), ep(cs.size());
  n_nodes = 0;
  n_samples = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint32_t N = 0, bins = 0;
    uint64_t first = 0, count = 0, chunk = 0, ns = 0;
    check_on(cs[i], epv_domain_stats_layout(cs[i], &N, &bins, &first, &count, &chunk), "epv_domain_stats_layout");
    check_on(cs[i], epv_domain_stats_samples(cs[i], &ns), "epv_domain_stats_samples");
    if (i == 0) { n_nodes = N; n_samples = ns; }
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of domain-statistics samples");
    else if (N != n_nodes) throw std::runtime_error("the contexts hold domain statistics of different trees");
    h[i].assign((size_t)N * 2u * EPV_DOM_BINS, 0u);
    l[i].assign((size_t)N * 2u, 0u);
    e[i].assign(std::max<size_t>((size_t)ns * N * 2u, 1u), 0u);
    check_on(cs[i], epv_get_domain_stats(cs[i], h[i].data(), l[i].data(), e[i].data()), "epv_get_domain_stats");
    hp[i] = h[i].data(); lp[i] = l[i].data(); ep[i] = e[i].data();
  }
  hist.assign((size_t)n_nodes * 2u * EPV_DOM_BINS, 0u);
  len_sum.assign((size_t)n_nodes * 2u, 0u);
  edges.assign((size_t)n_samples * n_nodes * 2u, 0u);
  std::vector<uint64_t> none(1, 0u);
  domain_parts_merge(cs.size(), n_nodes, n_samples, hp.data(), lp.data(), ep.data(), hist.data(), len_sum.data(),
                     edges.empty() ? none.data() : edges.data());
}

void SingleSiteSampler::download_domain_stats(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum,
                                              uint32_t &n_nodes, uint64_t &n_samples) {
  if (rank_mode_)
    throw std::runtime_error("download_domain_stats: this process holds one slot's stretch of the genome, not the genome: "
                             "merge the processes' download_domain_part in genome order (epv::domain_parts_merge, "
                             "epvh_domain_parts_merge), then close the merged part");
  std::vector<uint64_t> edges;
  download_domain_part(hist, len_sum, edges, n_nodes, n_samples);
  domain_part_close(n_nodes, n_samples, hist.data(), len_sum.data(), edges.data());
}

void SingleSiteSampler::set_domain_turnover(uint64_t max_samples) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || !max_samples)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_domain_turnover(c, max_samples), "epv_set_domain_turnover");
  turnover_max_ = max_samples;
}

void SingleSiteSampler::reset_domain_turnover() {
  if (!turnover_max_) throw std::runtime_error("domain turnover is off: set_domain_turnover first");
  for (epv_ctx *c : contexts()) check_on(c, epv_reset_domain_turnover(c), "epv_reset_domain_turnover");
}

void SingleSiteSampler::accumulate_domain_turnover() {
  if (!turnover_max_) throw std::runtime_error("domain turnover is off: set_domain_turnover first");
  for (epv_ctx *c : contexts()) check_on(c, epv_accumulate_domain_turnover(c), "epv_accumulate_domain_turnover");
}

void SingleSiteSampler::download_domain_turnover_part(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum,
                                                      std::vector<uint64_t> &edges, uint32_t &n_rows,
                                                      uint64_t &n_samples) {
  if (!turnover_max_) throw std::runtime_error("domain turnover is off: set_domain_turnover first");
  const std::vector<epv_ctx *> cs = contexts();   // in genome order
  std::vector<std::vector<uint64_t>> h(cs.size()), l(cs.size()), e(cs.size());
  std::vector<const uint64_t *> hp(cs.size()), lp(cs.size()), ep(cs.size());
  n_rows = 0;
  n_samples = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint32_t R = 0, bins = 0;
    uint64_t first = 0, count = 0, chunk = 0, ns = 0;
    check_on(cs[i], epv_domain_turnover_layout(cs[i], &R, &bins, &first, &count, &chunk), "epv_domain_turnover_layout");
    check_on(cs[i], epv_domain_turnover_samples(cs[i], &ns), "epv_domain_turnover_samples");
    if (i == 0) { n_rows = R; n_samples = ns; }
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of domain-turnover samples");
    else if (R != n_rows) throw std::runtime_error("the contexts hold domain turnover of different trees");
    h[i].assign((size_t)R * 4u * EPV_DOM_BINS, 0u);
    l[i].assign((size_t)R * 4u, 0u);
    e[i].assign(std::max<size_t>((size_t)ns * R * 2u, 1u), 0u);
    check_on(cs[i], epv_get_domain_turnover(cs[i], h[i].data(), l[i].data(), e[i].data()), "epv_get_domain_turnover");
    hp[i] = h[i].data(); lp[i] = l[i].data(); ep[i] = e[i].data();
  }
  hist.assign((size_t)n_rows * 4u * EPV_DOM_BINS, 0u);
  len_sum.assign((size_t)n_rows * 4u, 0u);
  edges.assign((size_t)n_samples * n_rows * 2u, 0u);
  std::vector<uint64_t> none(1, 0u);
  turnover_parts_merge(cs.size(), n_rows, n_samples, hp.data(), lp.data(), ep.data(), hist.data(), len_sum.data(),
                       edges.empty() ? none.data() : edges.data());
}

void SingleSiteSampler::download_domain_turnover(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum,
                                                 uint32_t &n_rows, uint64_t &n_samples) {
  if (rank_mode_)
    throw std::runtime_error("download_domain_turnover: this process holds one slot's stretch of the genome, not the "
                             "genome: merge the processes' download_domain_turnover_part in genome order "
                             "(epv::turnover_parts_merge, epvh_turnover_parts_merge), then close the merged part");
  std::vector<uint64_t> edges;
  download_domain_turnover_part(hist, len_sum, edges, n_rows, n_samples);
  turnover_part_close(n_rows, n_samples, hist.data(), len_sum.data(), edges.data());
}

void SingleSiteSampler::set_change_tracts(uint64_t max_samples) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || !max_samples)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_change_tracts(c, max_samples), "epv_set_change_tracts");
  tracts_max_ = max_samples;
}

void SingleSiteSampler::reset_change_tracts() {
  if (!tracts_max_) throw std::runtime_error("change tracts are off: set_change_tracts first");
  for (epv_ctx *c : contexts()) check_on(c, epv_reset_change_tracts(c), "epv_reset_change_tracts");
}

void SingleSiteSampler::accumulate_change_tracts() {
  if (!tracts_max_) throw std::runtime_error("change tracts are off: set_change_tracts first");
  for (epv_ctx *c : contexts()) check_on(c, epv_accumulate_change_tracts(c), "epv_accumulate_change_tracts");
}

void SingleSiteSampler::download_change_tracts_part(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum,
                                                    std::vector<uint64_t> &edges, uint32_t &n_branches,
                                                    uint64_t &n_samples) {
  if (!tracts_max_) throw std::runtime_error("change tracts are off: set_change_tracts first");
  const std::vector<epv_ctx *> cs = contexts();   // in genome order
  std::vector<std::vector<uint64_t>> h(cs.size()), l(cs.size()), e(cs.size());
  std::vector<const uint64_t *> hp(cs.size()), lp(cs.size()), ep(cs.size());
  n_branches = 0;
  n_samples = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint32_t B = 0, classes = 0, bins = 0;
    uint64_t first = 0, count = 0, chunk = 0, ns = 0;
    check_on(cs[i], epv_change_tracts_layout(cs[i], &B, &classes, &bins, &first, &count, &chunk), "epv_change_tracts_layout");
    check_on(cs[i], epv_change_tracts_samples(cs[i], &ns), "epv_change_tracts_samples");
    if (i == 0) { n_branches = B; n_samples = ns; }
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of change-tract samples");
    else if (B != n_branches) throw std::runtime_error("the contexts hold change tracts of different trees");
    h[i].assign((size_t)B * EPV_TRACT_CLASSES * EPV_DOM_BINS, 0u);
    l[i].assign((size_t)B * EPV_TRACT_CLASSES, 0u);
    e[i].assign(std::max<size_t>((size_t)ns * B * 2u, 1u), 0u);
    check_on(cs[i], epv_get_change_tracts(cs[i], h[i].data(), l[i].data(), e[i].data()), "epv_get_change_tracts");
    hp[i] = h[i].data(); lp[i] = l[i].data(); ep[i] = e[i].data();
  }
  hist.assign((size_t)n_branches * EPV_TRACT_CLASSES * EPV_DOM_BINS, 0u);
  len_sum.assign((size_t)n_branches * EPV_TRACT_CLASSES, 0u);
  edges.assign((size_t)n_samples * n_branches * 2u, 0u);
  std::vector<uint64_t> none(1, 0u);
  tract_parts_merge(cs.size(), n_branches, n_samples, hp.data(), lp.data(), ep.data(), hist.data(), len_sum.data(),
                    edges.empty() ? none.data() : edges.data());
}

void SingleSiteSampler::download_change_tracts(std::vector<uint64_t> &hist, std::vector<uint64_t> &len_sum,
                                               uint32_t &n_branches, uint64_t &n_samples) {
  if (rank_mode_)
    throw std::runtime_error("download_change_tracts: this process holds one slot's stretch of the genome, not the "
                             "genome: merge the processes' download_change_tracts_part in genome order "
                             "(epv::tract_parts_merge, epvh_tract_parts_merge), then close the merged part");
  std::vector<uint64_t> edges;
  download_change_tracts_part(hist, len_sum, edges, n_branches, n_samples);
  tract_part_close(n_branches, n_samples, hist.data(), len_sum.data(), edges.data());
}

void SingleSiteSampler::set_spatial_correlation(uint32_t max_lag, uint64_t max_samples) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || !max_lag)
    for (epv_ctx *c : contexts())
      check_on(c, epv_set_spatial_correlation(c, max_lag, max_samples), "epv_set_spatial_correlation");
  corr_lag_ = max_lag;
  corr_max_ = max_lag ? max_samples : 0u;
}

void SingleSiteSampler::reset_spatial_correlation() {
  if (!corr_lag_) throw std::runtime_error("spatial correlations are off: set_spatial_correlation first");
  for (epv_ctx *c : contexts()) check_on(c, epv_reset_spatial_correlation(c), "epv_reset_spatial_correlation");
}

void SingleSiteSampler::accumulate_spatial_correlation() {
  if (!corr_lag_) throw std::runtime_error("spatial correlations are off: set_spatial_correlation first");
  for (epv_ctx *c : contexts()) check_on(c, epv_accumulate_spatial_correlation(c), "epv_accumulate_spatial_correlation");
}

void SingleSiteSampler::download_spatial_correlation_part(std::vector<uint64_t> &n11, std::vector<uint64_t> &edges,
                                                          uint32_t &n_rows, uint32_t &max_lag, uint64_t &n_samples,
                                                          uint64_t &n_sites) {
  if (!corr_lag_) throw std::runtime_error("spatial correlations are off: set_spatial_correlation first");
  const std::vector<epv_ctx *> cs = contexts();   // in genome order
  std::vector<std::vector<uint64_t>> a(cs.size()), e(cs.size());
  std::vector<const uint64_t *> ap(cs.size()), ep(cs.size());
  std::vector<uint64_t> cnts(cs.size(), 0u);
  n_rows = 0;
  max_lag = corr_lag_;
  n_samples = 0;
  const uint32_t LW = corr_edge_words(corr_lag_);
  for (size_t i = 0; i < cs.size(); ++i) {
    uint32_t R = 0, L = 0;
    uint64_t first = 0, count = 0, chunk = 0, ns = 0;
    check_on(cs[i], epv_spatial_correlation_layout(cs[i], &R, &L, &first, &count, &chunk), "epv_spatial_correlation_layout");
    check_on(cs[i], epv_spatial_correlation_samples(cs[i], &ns), "epv_spatial_correlation_samples");
    if (L != corr_lag_) throw std::runtime_error("a context holds spatial correlations of another max_lag");
    if (i == 0) { n_rows = R; n_samples = ns; }
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of spatial-correlation samples");
    else if (R != n_rows) throw std::runtime_error("the contexts hold spatial correlations of different trees");
    cnts[i] = count;
    a[i].assign((size_t)R * (L + 1u), 0u);
    e[i].assign(std::max<size_t>((size_t)ns * R * 2u * LW, 1u), 0u);
    check_on(cs[i], epv_get_spatial_correlation(cs[i], a[i].data(), e[i].data()), "epv_get_spatial_correlation");
    ap[i] = a[i].data(); ep[i] = e[i].data();
  }
  n11.assign((size_t)n_rows * (max_lag + 1u), 0u);
  edges.assign(std::max<size_t>((size_t)n_samples * n_rows * 2u * LW, 1u), 0u);
  n_sites = corr_parts_merge(cs.size(), n_rows, max_lag, n_samples, cnts.data(), ap.data(), ep.data(), n11.data(),
                             edges.data());
  edges.resize((size_t)n_samples * n_rows * 2u * LW);
}

void SingleSiteSampler::download_spatial_correlation(std::vector<uint64_t> &n11, std::vector<uint64_t> &left1,
                                                     std::vector<uint64_t> &right1, uint32_t &n_rows,
                                                     uint32_t &max_lag, uint64_t &n_samples) {
  if (rank_mode_)
    throw std::runtime_error("download_spatial_correlation: this process holds one slot's stretch of the genome, not "
                             "the genome: merge the processes' download_spatial_correlation_part in genome order "
                             "(epv::corr_parts_merge, epvh_corr_parts_merge), then close the merged part");
  std::vector<uint64_t> edges;
  uint64_t n_sites = 0;
  download_spatial_correlation_part(n11, edges, n_rows, max_lag, n_samples, n_sites);
  left1.assign(n11.size(), 0u);
  right1.assign(n11.size(), 0u);
  std::vector<uint64_t> none(1, 0u);
  corr_part_close(n_rows, max_lag, n_samples, n_sites, n11.data(), edges.empty() ? none.data() : edges.data(),
                  left1.data(), right1.data());
}

void SingleSiteSampler::set_domain_maps(const std::vector<uint32_t> &sizes, uint32_t state, uint64_t max_samples) {
  if (!sizes.empty()) check_domain_map_sizes((uint32_t)sizes.size(), sizes.data(), "set_domain_maps");
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || sizes.empty())
    for (epv_ctx *c : contexts())
      check_on(c, epv_set_domain_maps(c, (uint32_t)sizes.size(), sizes.data(), state, max_samples), "epv_set_domain_maps");
  dmaps_sizes_ = sizes;
  dmaps_state_ = state;
  dmaps_max_ = sizes.empty() ? 0u : max_samples;
}

void SingleSiteSampler::reset_domain_maps() {
  if (dmaps_sizes_.empty()) throw std::runtime_error("domain maps are off: set_domain_maps first");
  for (epv_ctx *c : contexts()) check_on(c, epv_reset_domain_maps(c), "epv_reset_domain_maps");
}

void SingleSiteSampler::accumulate_domain_maps() {
  if (dmaps_sizes_.empty()) throw std::runtime_error("domain maps are off: set_domain_maps first");
  for (epv_ctx *c : contexts()) check_on(c, epv_accumulate_domain_maps(c), "epv_accumulate_domain_maps");
}

void SingleSiteSampler::download_domain_maps(std::vector<uint32_t> &counts, std::vector<uint64_t> &edges, uint32_t &n_nodes,
                                             uint64_t &n_samples, uint64_t &n_sites) {
  if (dmaps_sizes_.empty()) throw std::runtime_error("domain maps are off: set_domain_maps first");
  const std::vector<epv_ctx *> cs = contexts();   // in genome order
  const uint32_t K = (uint32_t)dmaps_sizes_.size(), EW = dmaps_edge_words(dmaps_sizes_.back());
  std::vector<std::vector<uint32_t>> a(cs.size());
  std::vector<std::vector<uint64_t>> e(cs.size());
  std::vector<const uint32_t *> ap(cs.size());
  std::vector<const uint64_t *> ep(cs.size());
  std::vector<uint64_t> cnts(cs.size(), 0u);
  n_nodes = 0;
  n_samples = n_sites = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint32_t N = 0, k = 0, state = 0, sizes[4] = {0, 0, 0, 0};
    uint64_t first = 0, count = 0, chunk = 0, ns = 0;
    check_on(cs[i], epv_domain_maps_layout(cs[i], &N, &k, sizes, &state, &first, &count, &chunk), "epv_domain_maps_layout");
    check_on(cs[i], epv_domain_maps_samples(cs[i], &ns), "epv_domain_maps_samples");
    if (k != K || !std::equal(dmaps_sizes_.begin(), dmaps_sizes_.end(), sizes) || state != dmaps_state_)
      throw std::runtime_error("a context holds domain maps of other sizes or another state");
    if (i == 0) { n_nodes = N; n_samples = ns; }
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of domain-map samples");
    else if (N != n_nodes) throw std::runtime_error("the contexts hold domain maps of different trees");
    cnts[i] = count;
    n_sites += count;
    a[i].assign(std::max<size_t>((size_t)N * K * count, 1u), 0u);
    e[i].assign(std::max<size_t>((size_t)ns * N * 2u * EW, 1u), 0u);
    check_on(cs[i], epv_get_domain_maps(cs[i], a[i].data(), e[i].data()), "epv_get_domain_maps");
    ap[i] = a[i].data(); ep[i] = e[i].data();
  }
  counts.assign(std::max<size_t>((size_t)n_nodes * K * n_sites, 1u), 0u);
  edges.assign(std::max<size_t>((size_t)n_samples * n_nodes * 2u * EW, 1u), 0u);
  domain_maps_merge(cs.size(), n_nodes, K, dmaps_sizes_.data(), n_samples, cnts.data(), ap.data(), ep.data(), counts.data(),
                    edges.data());
  counts.resize((size_t)n_nodes * K * n_sites);
  edges.resize((size_t)n_samples * n_nodes * 2u * EW);
}

void SingleSiteSampler::set_epoch_stats(uint32_t P) {
  // (before the first reset(model, tree, paths): applied to the contexts that reset builds)
  if (n_sites_ || !P)
    for (epv_ctx *c : contexts()) check_on(c, epv_set_epoch_stats(c, P), "epv_set_epoch_stats");
  epoch_P_ = P;
}

void SingleSiteSampler::download_epoch_stats(std::vector<uint64_t> &closed, std::vector<int> &k,
                                             std::vector<uint64_t> &fixT, uint64_t &n_samples) {
  if (!epoch_P_) throw std::runtime_error("epoch statistics are off: set_epoch_stats first");
  const std::vector<epv_ctx *> cs = contexts();
  const uint64_t B = (uint64_t)n_nodes_ - 1u, P = epoch_P_;
  n_samples = 0;
  for (size_t i = 0; i < cs.size(); ++i) {
    uint64_t ns = 0;
    if (epv_epoch_stats_samples(cs[i], &ns) != EPV_OK) throw std::runtime_error("epv_epoch_stats_samples failed");
    if (i == 0) n_samples = ns;
    else if (ns != n_samples) throw std::runtime_error("the contexts hold different numbers of epoch-statistics samples");
  }
  k.assign((size_t)n_nodes_, 0);
  fixT.assign((size_t)n_nodes_, 0u);
  uint32_t gotB = 0, gotP = 0;
  check_on(cs.at(0), epv_epoch_stats_layout(cs[0], &gotB, &gotP, k.data() + 1, fixT.data() + 1), "epv_epoch_stats_layout");
  if (gotB != B || gotP != P) throw std::runtime_error("the epoch statistics of the context have another layout");
  // every context's raw part, added as integers: part = lo + 2^32 hi is kept with lo < 2^32, so no word wraps
  std::vector<uint64_t> raw(B * P * 32u, 0u), part(B * P * 32u);
  for (epv_ctx *c : cs) {
    check_on(c, epv_get_epoch_stats(c, part.data()), "epv_get_epoch_stats");
    for (uint64_t cell = 0; cell < B * P; ++cell) {
      uint64_t *r = raw.data() + cell * 32u;
      const uint64_t *q = part.data() + cell * 32u;
      for (int c8 = 0; c8 < 8; ++c8) {
        r[c8] += q[c8];
        r[24 + c8] += q[24 + c8];           // (two's complement)
        const uint64_t lo = r[8 + c8] + (q[8 + c8] & 0xffffffffull);
        r[16 + c8] += q[16 + c8] + (q[8 + c8] >> 32) + (lo >> 32);
        r[8 + c8] = lo & 0xffffffffull;
      }
    }
  }
  closed.assign(B * P * 24u, 0u);
  if (B) epoch_close(raw.data(), fixT.data() + 1, (uint32_t)B, (uint32_t)P, closed.data());
}

void SingleSiteSampler::epoch_counts_to_stats(const std::vector<uint64_t> &closed, const std::vector<int> &k,
                                              uint64_t n_samples, std::vector<double> &J, std::vector<double> &D) const {
  const uint64_t B = (uint64_t)n_nodes_ - 1u, P = epoch_P_;
  if (closed.size() != B * P * 24u || k.size() != (size_t)n_nodes_)
    throw std::runtime_error("epoch_counts_to_stats: counts of the wrong size");
  J.assign(B * P * 8u, 0.0);
  D.assign(B * P * 8u, 0.0);
  if (B && P) epv::epoch_counts_to_stats(closed.data(), k.data() + 1, (uint32_t)B, (uint32_t)P, n_samples, J.data(), D.data());
}

void SingleSiteSampler::set_unobserved(std::vector<uint8_t> whole_genome) {
  bool any = false;
  for (uint8_t v : whole_genome) any = any || v != 0u;
  if (!any) whole_genome.clear();
  if (n_sites_ && !whole_genome.empty() && whole_genome.size() != (uint64_t)(n_nodes_ - 1) * n_sites_)
    throw std::runtime_error("mask of unobserved cells: " + std::to_string(whole_genome.size()) + " entries for " +
                             std::to_string(n_nodes_ - 1) + " branches x " + std::to_string(n_sites_) + " sites");
  unobs_ = std::move(whole_genome);
  if (!n_sites_) return;   // no paths yet: the reset that uploads them applies it
  if (!sharded()) {
    apply_unobserved(ctx_, 0, n_sites_);
    return;
  }
  for (const Part &p : parts_) apply_unobserved(p.ctx, p.lo, p.hi);
}

void SingleSiteSampler::apply_unobserved(epv_ctx *c, uint64_t lo, uint64_t hi) {
  if (unobs_.empty()) {
    check_on(c, epv_set_unobserved(c, nullptr), "epv_set_unobserved");
    return;
  }
  const uint64_t B = (uint64_t)n_nodes_ - 1u, w = hi - lo;
  std::vector<uint8_t> win(B * w);
  for (uint64_t b = 0; b < B; ++b)
    std::copy(unobs_.begin() + b * n_sites_ + lo, unobs_.begin() + b * n_sites_ + hi, win.begin() + b * w);
  check_on(c, epv_set_unobserved(c, win.data()), "epv_set_unobserved");
}

void SingleSiteSampler::set_regions(std::vector<uint64_t> lengths) {
  regions_ = std::move(lengths);
  if (!n_sites_) return;   // no paths yet: the reset that uploads them applies it
  build_fixed(n_sites_);
  if (!sharded()) {
    apply_fixed(ctx_, 0, n_sites_);
    return;
  }
  for (const Part &p : parts_) apply_fixed(p.ctx, p.lo, p.hi);
}

void SingleSiteSampler::build_fixed(uint64_t n) {
  fixed_.clear();
  n_fixed_ = 0;
  if (regions_.empty()) return;
  uint64_t total = 0;
  for (size_t k = 0; k < regions_.size(); ++k) {
    if (regions_[k] < 3)
      throw std::runtime_error("region " + std::to_string(k) + " holds " + std::to_string(regions_[k]) +
                               " sites, a region holds at least 3");
    total += regions_[k];
  }
  if (total != n)
    throw std::runtime_error("the regions hold " + std::to_string(total) + " sites in all, the paths hold " + std::to_string(n));
  fixed_.assign(n, 0);
  uint64_t a = 0;
  for (uint64_t m : regions_) {
    fixed_[a] = fixed_[a + m - 1] = 1;
    a += m;
  }
  for (uint64_t s = 1; s + 1 < n; ++s) n_fixed_ += fixed_[s];
}

void SingleSiteSampler::apply_fixed(epv_ctx *c, uint64_t lo, uint64_t hi) {
  check_on(c, epv_set_fixed_sites(c, fixed_.empty() ? nullptr : fixed_.data() + lo), "epv_set_fixed_sites");
  (void)hi;
}

void SingleSiteSampler::set_leaf_evidence(std::vector<float> whole_genome) {
  bool any = false;
  for (float r : whole_genome) any = any || r == r;
  if (!any) whole_genome.clear();
  if (n_sites_ && !whole_genome.empty() && whole_genome.size() != (uint64_t)(n_nodes_ - 1) * n_sites_)
    throw std::runtime_error("table of leaf evidence: " + std::to_string(whole_genome.size()) + " entries for " +
                             std::to_string(n_nodes_ - 1) + " branches x " + std::to_string(n_sites_) + " sites");
  evidence_ = std::move(whole_genome);
  if (!n_sites_) return;   // no paths yet: the reset that uploads them applies it
  if (!sharded()) {
    apply_leaf_evidence(ctx_, 0, n_sites_);
    return;
  }
  for (const Part &p : parts_) apply_leaf_evidence(p.ctx, p.lo, p.hi);
}

void SingleSiteSampler::apply_leaf_evidence(epv_ctx *c, uint64_t lo, uint64_t hi) {
  if (evidence_.empty()) {
    check_on(c, epv_set_leaf_evidence(c, nullptr), "epv_set_leaf_evidence");
    return;
  }
  const uint64_t B = (uint64_t)n_nodes_ - 1u, w = hi - lo;
  std::vector<float> win(B * w);
  for (uint64_t b = 0; b < B; ++b)
    std::copy(evidence_.begin() + b * n_sites_ + lo, evidence_.begin() + b * n_sites_ + hi, win.begin() + b * w);
  check_on(c, epv_set_leaf_evidence(c, win.data()), "epv_set_leaf_evidence");
}

void SingleSiteSampler::build(const Tree &th, const FlatPaths &paths, uint64_t n, bool rank_mode) {
  if (!evidence_.empty() && evidence_.size() != (uint64_t)(th.n_nodes() - 1) * n)
    throw std::runtime_error("table of leaf evidence: " + std::to_string(evidence_.size()) + " entries for " +
                             std::to_string(th.n_nodes() - 1) + " branches x " + std::to_string(n) + " sites");
  if (!unobs_.empty() && unobs_.size() != (uint64_t)(th.n_nodes() - 1) * n)
    throw std::runtime_error("mask of unobserved cells: " + std::to_string(unobs_.size()) + " entries for " +
                             std::to_string(th.n_nodes() - 1) + " branches x " + std::to_string(n) + " sites");
  build_fixed(n);   // (throws when the regions do not sum to this genome)
  n_nodes_ = th.n_nodes();
  n_sites_ = n;
  drop_parts();
  const uint64_t H = halo_for(burn_in, batch);
  const uint64_t min_part = 2 * H + 2 * kBlock;
  // slots: as many of the requested GPUs as the genome can feed, cut on multiples of 256 * row_blocks_ sites
  const std::vector<uint64_t> cut = shard_cuts(n, rank_mode ? world_ : devices_.size(), burn_in, batch, row_blocks_);
  const size_t G = cut.size() - 1;
  if (rank_mode && G != world_)
    throw std::runtime_error("a genome of " + std::to_string(n) + " sites cannot feed " + std::to_string(world_) + " GPU slots");
  world_ = G;
  // the slots that live in this process, and the columns of the genome `paths` holds
  const size_t g_lo = rank_mode ? (size_t)rank_.rank : 0, g_hi = rank_mode ? (size_t)rank_.rank + 1 : G;
  const uint64_t held_first = rank_mode ? cut[g_lo] : 0;
  if (rank_mode && paths.n_sites != cut[g_lo + 1] - cut[g_lo])
    throw std::runtime_error("slot " + std::to_string(g_lo) + " owns " + std::to_string(cut[g_lo + 1] - cut[g_lo]) +
                             " columns (shard_cuts), got " + std::to_string(paths.n_sites));
  struct Piece { size_t slot; uint64_t a, b; };
  std::vector<Piece> pieces;
  for (size_t g = g_lo; g < g_hi; ++g) {
    const uint64_t len = cut[g + 1] - cut[g];
    size_t k = (size_t)contexts_per_gpu();
    while (k > 1 && len < k * min_part) --k;
    for (size_t j = 0; j < k; ++j) {
      const uint64_t a = j == 0 ? cut[g] : cut[g] + round_to((double)j * (double)len / (double)k, kBlock);
      const uint64_t b = j + 1 == k ? cut[g + 1] : cut[g] + round_to((double)(j + 1) * (double)len / (double)k, kBlock);
      pieces.push_back({g - g_lo, a, b});
    }
  }
  if (pieces.size() == 1 && G == 1 && !force_comm_) {
    check(epv_set_tree(ctx_, th.n_nodes(), th.parent_ids.data(), th.subtree_sizes.data(),
                       th.branches.data()), "epv_set_tree");
    check(epv_upload_paths(ctx_, paths.n_sites, paths.init.data(), paths.offsets.data(),
                           paths.jumps.data(), capacity_, 0), "epv_upload_paths");
    if (!unobs_.empty()) apply_unobserved(ctx_, 0, n);
    if (!evidence_.empty()) apply_leaf_evidence(ctx_, 0, n);
    if (!fixed_.empty()) apply_fixed(ctx_, 0, n);
    return;
  }
  uint32_t cap = capacity_;
  if (cap == 0) {   // the library's default rule, evaluated once for the whole genome
    if (rank_mode) {
      cap = 16;     // the slots cannot see each other's inputs: start narrow, widen on demand like every overflow
    } else {
      uint64_t maxj = 0;
      for (size_t e = 0; e + 1 < paths.offsets.size(); ++e) maxj = std::max(maxj, paths.offsets[e + 1] - paths.offsets[e]);
      cap = (uint32_t)std::min<uint64_t>(kMaxCap, std::max<uint64_t>(16, 2 * maxj + 8));
    }
  }
  if (rank_mode) {   // every slot must propose under one capacity: at least what its own input needs
    uint64_t maxj = 0;
    for (size_t e = 0; e + 1 < paths.offsets.size(); ++e) maxj = std::max(maxj, paths.offsets[e + 1] - paths.offsets[e]);
    if (maxj > cap) throw std::runtime_error("one slot per process: pass a capacity of at least " + std::to_string(maxj));
  }
  halo_ = H;
  slots_.resize(g_hi - g_lo);
  for (size_t g = g_lo; g < g_hi; ++g) {
    Slot &sl = slots_[g - g_lo];
    sl.device = devices_[g - g_lo];
    sl.gidx = g;
    sl.first = cut[g];
    sl.last = cut[g + 1];
  }
  const size_t P = pieces.size();
  for (size_t p = 0; p < P; ++p) {
    Part q;
    q.slot = pieces[p].slot;
    q.a = pieces[p].a;
    q.b = pieces[p].b;
    q.lo = q.a - (q.a > 0 ? H : 0);
    q.hi = q.b + (q.b < n ? H : 0);
    if (p == 0) {
      q.ctx = ctx_;
    } else {
      q.ctx = epv_create(slots_[q.slot].device);
      if (!q.ctx)
        throw std::runtime_error("cannot open a context on HIP device " + std::to_string(slots_[q.slot].device));
    }
    if (parts_.empty() || parts_.back().slot != q.slot) slots_[q.slot].part0 = parts_.size();
    slots_[q.slot].part1 = parts_.size() + 1;
    parts_.push_back(q);
    epv_ctx *c = q.ctx;
    check_on(c, epv_set_tree(c, th.n_nodes(), th.parent_ids.data(), th.subtree_sizes.data(), th.branches.data()),
             "epv_set_tree");
    check_on(c, epv_set_options(c, options_), "epv_set_options");   // (a context made here starts with none)
    const FlatPaths part = slice_sites_padded(paths, held_first, q.lo, q.hi);
    const double dummy = 0.0;
    check_on(c, epv_upload_paths(c, part.n_sites, part.init.data(), part.offsets.data(),
                                 part.jumps.empty() ? &dummy : part.jumps.data(), cap, q.lo), "epv_upload_paths");
    if (!unobs_.empty()) apply_unobserved(c, q.lo, q.hi);   // (its window of the genome, halos included)
    if (!evidence_.empty()) apply_leaf_evidence(c, q.lo, q.hi);
    if (!fixed_.empty()) apply_fixed(c, q.lo, q.hi);
    check_on(c, epv_set_global_length(c, n), "epv_set_global_length");
  }
  if (rank_mode) {
    // one communicator rank in this process, made once (an RCCL id serves one ncclCommInitRank)
    if (!rank_comm_ && epv_comm_init_rank(rank_.device, rank_.world, rank_.rank, rank_.id, &rank_comm_) != EPV_OK)
      throw std::runtime_error("cannot join the RCCL communicator as rank " + std::to_string(rank_.rank) + " of " +
                               std::to_string(rank_.world));
    slots_[0].comm = rank_comm_;
  } else if (G > 1 || force_comm_) {
    // one communicator rank per slot, all driven from this process: RCCL over the node's xGMI
    // links when the devices are distinct, the loopback transport when they repeat
    std::vector<int> devs(G);
    std::vector<epv_comm *> comms(G, nullptr);
    for (size_t g = 0; g < G; ++g) devs[g] = slots_[g].device;
    if (epv_comm_init_all((int)G, devs.data(), comms.data()) != EPV_OK)
      throw std::runtime_error("cannot set up the RCCL communicator over " + std::to_string(G) + " GPU slot(s)");
    for (size_t g = 0; g < G; ++g) slots_[g].comm = comms[g];
  }
}

void SingleSiteSampler::init_paths_indep(const Model &m, const Tree &th, const std::vector<uint8_t> &root_seq,
                                         const std::vector<uint8_t> &leaf_seq, uint64_t seed) {
  if (root_seq.size() != leaf_seq.size()) throw std::runtime_error("sequences differ in length");
  drop_parts();   // epievo_sim_pairwise's path runs on one context
  n_nodes_ = th.n_nodes();
  n_sites_ = root_seq.size();
  check(epv_set_tree(ctx_, th.n_nodes(), th.parent_ids.data(), th.subtree_sizes.data(),
                     th.branches.data()), "epv_set_tree");
  check(epv_set_model(ctx_, m.rates.data(), m.T.data()), "epv_set_model");
  check(epv_init_paths_indep(ctx_, root_seq.size(), root_seq.data(), leaf_seq.data(), seed, capacity_),
        "epv_init_paths_indep");
  check(epv_reset(ctx_), "epv_reset");
}

void SingleSiteSampler::reset(const Model &m) {
  apply_sample_root();
  if (!sharded()) {
    check(epv_set_model(ctx_, m.rates.data(), m.T.data()), "epv_set_model");
    check(epv_reset(ctx_), "epv_reset");
    return;
  }
  for (Part &p : parts_) check_on(p.ctx, epv_set_model(p.ctx, m.rates.data(), m.T.data()), "epv_set_model");
  refresh_parts();
  // the parts' cached likelihoods: launched on every part's stream, not waited for -- the MCMC calls
  // that follow queue up behind them (reset -> run_mcmc is how the EM loop goes,
  // epievo_est_params_histories.cpp:241-248), download() and the other readers synchronise anyway
  for (Part &p : parts_) check_on(p.ctx, epv_reset_async(p.ctx), "epv_reset_async");
}

// a slot's piece of the statistics all-gather: its counts [batch][16 B], then this tail
// {accepted proposals, widest jump capacity of its contexts}
static const uint64_t kTail = 2;

void SingleSiteSampler::ensure_stat_buffers() {
  if (!slots_[0].comm || (stat_batch_ == batch && slots_[0].d_piece)) return;
  free_stat_buffers();
  const uint64_t bytes = (batch * ((uint64_t)n_nodes_ - 1) * 16 + kTail) * sizeof(int64_t);
  for (Slot &s : slots_) {
    epv_ctx *c = parts_[s.part0].ctx;
    check_on(c, epv_dev_alloc(c, bytes, &s.d_piece), "epv_dev_alloc");
    check_on(c, epv_dev_alloc(c, world_ * bytes, &s.d_gather), "epv_dev_alloc");
  }
  stat_batch_ = batch;
}

void SingleSiteSampler::run_mcmc(uint64_t seed, uint64_t em_iteration,
                                 std::vector<std::vector<double>> &J,
                                 std::vector<std::vector<double>> &D, double &acceptance_rate) {
  apply_sample_root();
  const size_t B = (size_t)n_nodes_ - 1;
  std::vector<double> Jf(B * 8), Df(B * 8);
  uint64_t n_acc = 0;
  const uint32_t base = (uint32_t)(em_iteration * (burn_in + batch));
  if (!sharded()) {
    check_mcmc(epv_run_mcmc(ctx_, burn_in, batch, seed, base, Jf.data(), Df.data(), &n_acc), "epv_run_mcmc");
  } else {
    ensure_stat_buffers();
    // one host thread per part (the persistent workers): their colour phases run concurrently, each GPU on
    // its own, the contexts of one GPU on their own streams
    const size_t P = parts_.size();
    const uint64_t words = batch * B * 16, piece = words + kTail;
    std::vector<int> rcs(P, EPV_OK);
    std::vector<uint64_t> acc(P, 0);
    std::vector<std::vector<int64_t>> counts(P, std::vector<int64_t>(words));
    on_parts([&](size_t p) {
      rcs[p] = epv_run_mcmc_counts(parts_[p].ctx, burn_in, batch, seed, base, counts[p].data(), &acc[p]);
    });
    for (size_t p = 0; p < P; ++p) {
      epv_ctx *c = parts_[p].ctx;
      if (rcs[p] == EPV_ERR_CAPACITY) {   // absorbed as in check_mcmc; refresh_parts() evens the widths out
        uint32_t cap = 0;
        if (epv_get_capacity(c, &cap) == EPV_OK && cap < kMaxCap) {
          capacity_events.push_back(std::string("epv_run_mcmc_counts: ") + epv_last_error(c));
          check_on(c, epv_set_capacity(c, std::min(kMaxCap, cap * 2u)), "epv_set_capacity");
          rcs[p] = EPV_OK;
        }
      }
      check_on(c, rcs[p], "epv_run_mcmc_counts");
    }
    // the piece of every slot that lives here: its parts' counts added as integers, and the tail
    // (a slot that absorbed an overflow widened its slots: every slot of the run must follow
    // before the next halo exchange, whose column size depends on it)
    std::vector<int64_t> pieces(slots_.size() * piece, 0);
    for (size_t i = 0; i < slots_.size(); ++i) {
      int64_t *mine = pieces.data() + i * piece;
      for (size_t p = slots_[i].part0; p < slots_[i].part1; ++p) {
        for (uint64_t k = 0; k < words; ++k) mine[k] += counts[p][k];
        mine[words] += (int64_t)acc[p];
        uint32_t cap = 0;
        check_on(parts_[p].ctx, epv_get_capacity(parts_[p].ctx, &cap), "epv_get_capacity");
        mine[words + 1] = std::max<int64_t>(mine[words + 1], cap);
      }
    }
    if (slots_[0].comm) {
      // the one collective of an EM iteration: every slot's piece to every slot
      for (size_t i = 0; i < slots_.size(); ++i) {
        epv_ctx *c = parts_[slots_[i].part0].ctx;
        check_on(c, epv_dev_write(c, slots_[i].d_piece, pieces.data() + i * piece, piece * sizeof(int64_t)),
                 "epv_dev_write");
      }
      if (epv_comm_group_start() != EPV_OK) throw std::runtime_error("epv_comm_group_start failed");
      for (Slot &s : slots_)
        check_comm(s.comm, epv_comm_all_gather(s.comm, s.d_piece, s.d_gather, piece * sizeof(int64_t)),
                   "epv_comm_all_gather");
      if (epv_comm_group_end() != EPV_OK) throw std::runtime_error("epv_comm_group_end failed (statistics all-gather)");
      for (Slot &s : slots_) check_comm(s.comm, epv_comm_sync(s.comm), "epv_comm_sync");
      // every GPU now holds the pieces of all slots; the host M-step needs one copy
      pieces.assign(world_ * piece, 0);
      check(epv_dev_read(ctx_, pieces.data(), slots_[0].d_gather, pieces.size() * sizeof(int64_t)), "epv_dev_read");
    }
    std::vector<int64_t> total(words, 0);
    int64_t cap_all = 0;
    for (size_t g = 0; g * piece < pieces.size(); ++g) {
      const int64_t *pc = pieces.data() + g * piece;
      for (uint64_t k = 0; k < words; ++k) total[k] += pc[k];
      n_acc += (uint64_t)pc[words];
      cap_all = std::max(cap_all, pc[words + 1]);
    }
    check(epv_counts_to_stats(ctx_, total.data(), batch, 1, Jf.data(), Df.data()), "epv_counts_to_stats");
    for (Part &q : parts_) {     // (slots in other processes may have grown)
      uint32_t cap = 0;
      check_on(q.ctx, epv_get_capacity(q.ctx, &cap), "epv_get_capacity");
      if (cap < cap_all) check_on(q.ctx, epv_set_capacity(q.ctx, (uint32_t)cap_all), "epv_set_capacity");
    }
  }
  J.assign(n_nodes_, {});
  D.assign(n_nodes_, {});
  for (size_t b = 1; b <= B; ++b) {
    J[b].assign(Jf.begin() + (b - 1) * 8, Jf.begin() + b * 8);
    D[b].assign(Df.begin() + (b - 1) * 8, Df.begin() + b * 8);
  }
  acceptance_rate = static_cast<double>(n_acc) / (batch * (n_sites_ - 2 - n_fixed_));
}

size_t SingleSiteSampler::sweeps(size_t n, uint64_t seed, uint32_t sweep_base) {
  apply_sample_root();
  uint64_t n_acc = 0;
  if (!sharded()) {
    check_mcmc(epv_sweep(ctx_, n, seed, sweep_base, &n_acc), "epv_sweep");
    return n_acc;
  }
  // a sharded genome can run as many sweeps as its halos last, then they are refreshed
  size_t done = 0;
  while (done < n) {
    uint64_t left = ~0ull;
    for (Part &p : parts_) { uint64_t v = 0; check_on(p.ctx, epv_halo_phases_left(p.ctx, &v), "epv_halo_phases_left"); left = std::min(left, v); }
    const size_t kk = std::min<size_t>(n - done, (size_t)(left / 3));
    if (kk == 0) {
      refresh_parts();
      for (Part &p : parts_) check_on(p.ctx, epv_reset(p.ctx), "epv_reset");
      continue;
    }
    const size_t P = parts_.size();
    std::vector<int> rcs(P, EPV_OK);
    std::vector<uint64_t> acc(P, 0);
    on_parts([&](size_t p) { rcs[p] = epv_sweep(parts_[p].ctx, kk, seed, sweep_base + (uint32_t)done, &acc[p]); });
    bool grew = false;
    for (size_t p = 0; p < P; ++p) {
      epv_ctx *c = parts_[p].ctx;
      if (rcs[p] == EPV_ERR_CAPACITY) {
        uint32_t cap = 0;
        if (epv_get_capacity(c, &cap) == EPV_OK && cap < kMaxCap) {
          capacity_events.push_back(std::string("epv_sweep: ") + epv_last_error(c));
          check_on(c, epv_set_capacity(c, std::min(kMaxCap, cap * 2u)), "epv_set_capacity");
          rcs[p] = EPV_OK;
          grew = true;
        }
      }
      check_on(c, rcs[p], "epv_sweep");
      n_acc += acc[p];
    }
    // the parts update their shared halo columns redundantly: they must keep proposing under
    // the same capacity, or one accepts what the other rejects
    if (grew) equalize_capacity();
    done += kk;
  }
  return n_acc;
}

void SingleSiteSampler::scale_jump_times(const std::vector<double> &new_branches) {
  if (!sharded()) { check(epv_scale_jump_times(ctx_, new_branches.data()), "epv_scale_jump_times"); return; }
  for (Part &p : parts_) check_on(p.ctx, epv_scale_jump_times(p.ctx, new_branches.data()), "epv_scale_jump_times");
}

void SingleSiteSampler::upload(const Tree &th, const FlatPaths &paths) {
  drop_parts();   // the site-independent stage runs on one context
  n_nodes_ = th.n_nodes();
  n_sites_ = paths.n_sites;
  check(epv_set_tree(ctx_, th.n_nodes(), th.parent_ids.data(), th.subtree_sizes.data(),
                     th.branches.data()), "epv_set_tree");
  // the kernels of the site-independent stage never read the 8 rates; park neutral ones
  const double ones[8] = {1, 1, 1, 1, 1, 1, 1, 1}, T[4] = {0.5, 0.5, 0.5, 0.5};
  check(epv_set_model(ctx_, ones, T), "epv_set_model");
  const double dummy = 0.0;
  check(epv_upload_paths(ctx_, paths.n_sites, paths.init.data(), paths.offsets.data(),
                         paths.jumps.empty() ? &dummy : paths.jumps.data(), capacity_, 0),
        "epv_upload_paths");
  // new paths cleared the context's tables: a mask or a table the sampler keeps goes back on, as in build()
  const uint64_t cells = (uint64_t)(n_nodes_ - 1) * n_sites_;
  if (!unobs_.empty() && unobs_.size() != cells)
    throw std::runtime_error("mask of unobserved cells: " + std::to_string(unobs_.size()) + " entries for " +
                             std::to_string(n_nodes_ - 1) + " branches x " + std::to_string(n_sites_) + " sites");
  if (!evidence_.empty() && evidence_.size() != cells)
    throw std::runtime_error("table of leaf evidence: " + std::to_string(evidence_.size()) + " entries for " +
                             std::to_string(n_nodes_ - 1) + " branches x " + std::to_string(n_sites_) + " sites");
  if (!unobs_.empty()) apply_unobserved(ctx_, 0, n_sites_);
  if (!evidence_.empty()) apply_leaf_evidence(ctx_, 0, n_sites_);
}

void SingleSiteSampler::get_sufficient_statistics(std::vector<std::vector<double>> &J,
                                                  std::vector<std::vector<double>> &D) {
  if (sharded()) throw std::runtime_error("get_sufficient_statistics: load the paths with upload() (one context)");
  const size_t B = (size_t)n_nodes_ - 1;
  std::vector<double> Jf(B * 8), Df(B * 8);
  check(epv_get_sufficient_statistics(ctx_, Jf.data(), Df.data()), "epv_get_sufficient_statistics");
  J.assign(n_nodes_, {});
  D.assign(n_nodes_, {});
  for (size_t b = 1; b <= B; ++b) {
    J[b].assign(Jf.begin() + (b - 1) * 8, Jf.begin() + b * 8);
    D[b].assign(Df.begin() + (b - 1) * 8, Df.begin() + b * 8);
  }
}

void SingleSiteSampler::indep_expectation(const double rates[2], std::vector<double> &J,
                                          std::vector<double> &D) {
  J.assign(((size_t)n_nodes_ - 1) * 2, 0.0);
  D.assign(((size_t)n_nodes_ - 1) * 2, 0.0);
  check(epv_indep_expectation(ctx_, rates, J.data(), D.data()), "epv_indep_expectation");
}

void SingleSiteSampler::indep_sufficient_statistics(std::vector<double> &J, std::vector<double> &D) {
  J.assign(((size_t)n_nodes_ - 1) * 2, 0.0);
  D.assign(((size_t)n_nodes_ - 1) * 2, 0.0);
  check(epv_indep_sufficient_statistics(ctx_, J.data(), D.data()), "epv_indep_sufficient_statistics");
}

void SingleSiteSampler::indep_node_posterior(const double rates[2], std::vector<double> &p_state1) {
  if (sharded()) throw std::runtime_error("indep_node_posterior: load the paths with upload() (one context)");
  p_state1.assign((size_t)n_nodes_ * n_sites_, 0.0);
  check(epv_indep_node_posterior(ctx_, rates, p_state1.data()), "epv_indep_node_posterior");
}

void SingleSiteSampler::indep_update_paths(const double rates[2], uint64_t seed, uint32_t sweep) {
  check_mcmc(epv_indep_update_paths(ctx_, rates, seed, sweep), "epv_indep_update_paths");
}

void SingleSiteSampler::download(FlatPaths &paths) {
  if (sharded()) {
    // every part on its own host thread (its context has its own stream): gather, copy, trim halos
    std::vector<FlatPaths> owned(parts_.size());
    std::vector<std::string> errors(parts_.size());
    on_parts([this, &owned, &errors](size_t i) {
        try {
          Part &q = parts_[i];
          epv_ctx *c = q.ctx;
          uint64_t total = 0;
          check_on(c, epv_paths_total_jumps(c, &total), "epv_paths_total_jumps");
          FlatPaths p;
          p.n_sites = q.hi - q.lo;
          p.n_nodes = n_nodes_;
          const uint64_t E = (uint64_t)(n_nodes_ - 1) * p.n_sites;
          p.init.assign(E, 0);
          p.offsets.assign(E + 1, 0);
          p.jumps.assign(total ? total : 1, 0.0);
          check_on(c, epv_download_paths(c, p.init.data(), p.offsets.data(), p.jumps.data()), "epv_download_paths");
          p.jumps.resize(total);
          owned[i] = slice_sites(p, q.a - q.lo, q.b - q.lo);
        } catch (const std::exception &e) { errors[i] = e.what(); }
      });
    for (const std::string &e : errors) if (!e.empty()) throw std::runtime_error(e);
    paths = concat_sites(owned);
    return;
  }
  uint64_t total = 0;
  check(epv_paths_total_jumps(ctx_, &total), "epv_paths_total_jumps");
  paths.n_sites = n_sites_;
  paths.n_nodes = n_nodes_;
  const uint64_t E = (uint64_t)(n_nodes_ - 1) * n_sites_;
  paths.init.assign(E, 0);
  paths.offsets.assign(E + 1, 0);
  paths.jumps.assign(total ? total : 1, 0.0);
  check(epv_download_paths(ctx_, paths.init.data(), paths.offsets.data(), paths.jumps.data()),
        "epv_download_paths");
  paths.jumps.resize(total);
}

}  // namespace epv
