// epv_abi.hip -- the extern "C" boundary of include/epievo_mi355x.h: device memory,
// stream, launches.  No torch types, no exceptions across the boundary, no CPU
// fallback: when HIP is unavailable every entry point fails with EPV_ERR_HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <new>
#include <vector>

#include "epievo_mi355x.h"
#include "epv_device.h"
#include "epv_plan.h"     // the colour phase: knobs, launch shapes, kernel variants (host only)
#include "epv_part.h"     // the parts of the summaries that are joint along the genome: every byte size (host only)

#define EPV_API extern "C" __attribute__((visibility("default")))

#include "epv_kernels.h"  // all __global__ kernels (single translation unit, no -fgpu-rdc)
#include "epv_math.h"
#include "epv_pavg.h"
#include "epv_bevents.h"
#include "epv_mixing.h"
#include "epv_wstat.h"
#include "epv_epochs.h"
#include "epv_origin.h"
#include "epv_domains.h"
#include "epv_turnover.h"
#include "epv_corr.h"
#include "epv_dmaps.h"
#include "epv_tracts.h"
#include "epv_patterns.h"
#include "epv_regions.h"   // fixed sites: the guards around a colour phase, the statistics correction

// ---- the state of the posterior summaries ("layers") of run_mcmc, one struct each.  Every member has a default:
// a layer goes off by freeing its device buffers and taking a default-constructed struct (the *_off functions).
// The sites a layer was laid out for: a layer whose current sites differ is laid out again, or, once it holds
// samples, refused (sites_changed).  A member a layer does not depend on stays zero on both sides of the comparison
struct SiteLayout {
  uint64_t lo = 0;       // first local site
  uint64_t cnt = 0;      // sites counted (the layers of pavg_range)
  uint64_t hi = 0;       // last local site (the layers of owned_range; hi < lo: none)
  uint64_t n = 0, g0 = 0, ng = 0;   // S.n, S.g0, S.n_global
  uint32_t B = 0;
  bool operator==(const SiteLayout &o) const {
    return lo == o.lo && cnt == o.cnt && hi == o.hi && n == o.n && g0 == o.g0 && ng == o.ng && B == o.B;
  }
};
// average history of the sampled paths (epv_pavg.h), off while P == 0
struct PavgState {
  uint32_t P = 0;
  int32_t *d = nullptr;            // [B][P][at.cnt] counts over local sites at.lo .. at.lo + at.cnt - 1
  SiteLayout at;                   // (without ng: the path average never depended on the genome's length)
  uint64_t samples = 0;
  double *d_grid = nullptr;        // [B][P] grid times
  std::vector<double> grid_blen;   // the branch lengths d_grid was built from
  uint32_t *d_out = nullptr;       // read-out staging
  uint64_t out_cap = 0;            // bytes
};
// posterior branch-event maps (epv_bevents.h), off while !on
struct BeventsState {
  bool on = false;
  uint32_t *d = nullptr;           // [6][B][at.cnt] counts over local sites at.lo .. at.lo + at.cnt - 1
  SiteLayout at;
  uint64_t samples = 0;
  unsigned long long *d_out = nullptr;   // window read-out staging
  uint64_t out_cap = 0;            // bytes
};
// regional sufficient statistics (epv_wstat.h), off while W == 0
struct WstatState {
  uint64_t W = 0;                  // sites per window, clamped to n_global
  uint64_t W_asked = 0;            // as epv_set_window_stats got it (a changed n_global clamps it again)
  unsigned long long *d = nullptr;   // [nw][B][16] over the global windows w0 .. w0 + nw - 1
  uint64_t w0 = 0, nw = 0;
  SiteLayout at;
  uint64_t samples = 0;
  std::vector<double> scale;       // 2^k_b of the first sample: the integers of later ones must mean the same
};
// epoch statistics (epv_epochs.h), off while P == 0.  No SiteLayout: the accumulator depends on B alone
struct EpochState {
  uint32_t P = 0;                  // epochs per branch
  unsigned long long *d = nullptr;   // [B][P][32]: J[8], lo[8], hi[8], cov[8]
  uint32_t B = 0;
  uint64_t samples = 0;
  uint64_t addends = 0;            // blocks along the sites, added over the samples: the addends a global word has received
  std::vector<double> scale;       // 2^k_b of the first sample: the integers of later ones must mean the same
  std::vector<uint64_t> fixT;      // llrint(T_b 2^k_b) of the first sample: the edges its epochs were cut at
};
// lineage origin maps (epv_origin.h), off while !on
struct OriginsState {
  bool on = false;
  uint32_t *d = nullptr;                  // origin [R][at.cnt] counts over local sites at.lo .. at.lo + at.cnt - 1
  unsigned long long *d_age = nullptr;    // age [L][at.cnt]
  SiteLayout at;                          // (without B: the tree is compared itself)
  uint32_t L = 0, R = 0;                  // leaves and rows of the tree they were laid out for
  uint64_t samples = 0;
  std::vector<uint32_t> parent;           // the tree of the tables below
  std::vector<uint32_t> first, leaf, rowb;   // first row per leaf [L + 1]; leaf and branch node per row [R]
  std::vector<long long> fixT;            // [N] llrint(ldexp(T_v, k)): with k what the accumulated ages mean
  int k = 0;
  uint32_t *d_first = nullptr, *d_rowb = nullptr;
  long long *d_fixT = nullptr;
  unsigned long long *d_out = nullptr;    // window read-out staging
  uint64_t out_cap = 0;                   // bytes
};
// What the five summaries that are joint along the genome keep (epv_part.h): a context counts a PART, the host
// merges the parts.  The sizes are those of the shape the part was laid out with; nothing computes them again
struct PartState {
  uint64_t max = 0;                       // samples the edge records are allocated for
  uint64_t samples = 0;
  SiteLayout at;                          // (with B only where the rows depend on nothing else of the tree)
  PartShape shape;                        // rows, words and every byte size below
  std::vector<uint32_t> tree;             // what of the tree the rows depend on (the layer's describe function)
  unsigned long long *d_bits = nullptr;   // [rows][words] scratch: the rows of one sample, 64 sites a word
  unsigned long long *d_edge = nullptr;   // [max] edge records of shape.edge_b bytes: what a sample's stretch cannot close
  void *d_acc[2] = {nullptr, nullptr};    // shape.acc_b bytes each: what the stretch closes, over the samples
};
// domain size spectra (epv_domains.h), off while !on: acc = hist [N][2][128], len [N][2]; edge [max][N][2]
struct DomainsState : PartState {
  bool on = false;
  uint32_t child0 = 0;                    // the root's lowest-numbered child
};

// change patterns (epv_patterns.h), off while !on
struct PatternsState {
  bool on = false;
  uint32_t *d = nullptr;                  // [R][at.cnt] counts over local sites at.lo .. at.lo + at.cnt - 1
  SiteLayout at;
  uint32_t I = 0, R = 0;                  // clade rows and all rows of the tree they were laid out for
  uint64_t samples = 0;
  std::vector<uint32_t> subtree;          // the tree's pre-order subtree sizes: what the row layout depends on
  unsigned long long *d_out = nullptr;    // window read-out staging
  uint64_t out_cap = 0;                   // bytes
};

// domain turnover (epv_turnover.h), off while !on: R = 2 B rows; acc = hist [R][2][2][128], len [R][2][2]; edge [max][R][2]
struct TurnoverState : PartState {
  bool on = false;
};

// spatial correlations (epv_corr.h), off while L == 0: R = N + B rows; acc = n11 [R][L + 1]; edge [max][R][2][LW]
struct CorrState : PartState {
  uint32_t L = 0;                         // max_lag
  uint32_t child0 = 0;                    // the root's lowest-numbered child: what row 0 depends on
};

// chain mixing diagnostics (epv_mixing.h), off while K == 0.  The one layer that is joint across samples: it keeps
// a run, the samples linked each to its predecessor
struct MixingState {
  uint32_t K = 0;                         // max_lag
  unsigned long long *d_fp = nullptr;     // [at.cnt] fingerprint of the site's history at the last sample
  uint32_t *d_moved = nullptr;            // [at.cnt] linked pairs whose histories differ
  unsigned long long *d_sums = nullptr;   // [2 + K][at.cnt] S1, S2, C_1 .. C_K
  uint32_t *d_ring = nullptr;             // [K][at.cnt] the last K values of x of the run
  SiteLayout at;                          // (with B)
  uint32_t C = 0;                         // the capacity the cap was last evaluated for
  uint64_t samples = 0, moved_pairs = 0;
  uint64_t pairs[EPV_MIX_MAX_LAG + 1u] = {};   // [k] linked pairs at lag k = 1 .. K
  bool run_open = false;                  // a fingerprint of the state one sweep back may be on the device
  uint64_t run_len = 0;                   // samples of the open run
  uint64_t run_sweep = 0;                 // n_sweeps at the run's last sample (or its opening state)
  unsigned long long *d_out = nullptr;    // window read-out staging
  uint64_t out_cap = 0;                   // bytes
};

// domain maps (epv_dmaps.h), off while Z.K == 0: N rows; acc = counts uint32 [N][K][at.cnt]; edge [max][N][2][EW]
struct DmapsState : PartState {
  EpvDmapSizes Z{};                       // the sizes
  uint32_t state = 1;                     // the state whose runs are located
  uint32_t child0 = 0;                    // the root's lowest-numbered child
};

// change tracts (epv_tracts.h), off while !on: the turnover's 2 B rows; acc = hist [B][27][128], len [B][27];
// edge [max][B][2]
struct TractsState : PartState {
  bool on = false;
};

// fixed sites (epv_set_fixed_sites; epv_regions.h).  Everything is empty while no site is fixed: no launch, no buffer
struct FixedState {
  std::vector<uint8_t> mask;     // the mask as set, n local columns
  uint64_t *d_sites = nullptr;   // the fixed local sites among 1 .. n - 2, colour by colour
  uint64_t off[4] = {0, 0, 0, 0};  // colour k: d_sites[off[k] .. off[k + 1])
  EpvFixedSave save{};           // what the guard keeps over a phase, one slot per listed site
};

struct epv_ctx {
  int device = 0;
  EpvKnobs knobs;
  hipStream_t stream = nullptr;
  std::string err;
  EpvDev S{};
  bool have_tree = false, have_model = false, have_paths = false, have_reset = false;
  // host copies
  std::vector<uint32_t> parent, subtree;
  std::vector<double> blen;
  EpvModelConst model{};
  uint64_t first = 0, last = 0;          // fixed update range (no halo mode)
  uint64_t halo_left = 0, halo_right = 0;  // halo mode: widths of the halo column blocks
  bool halo_mode = false;
  uint64_t phases_used = 0;              // colour phases run since the halos were fresh
  // device allocations
  EpvModelConst *d_model = nullptr;
  // epv_set_model is stream-ordered: the constants leave from one of two pinned slots, taken in turn; a slot is
  // written again only after the copy that last read it has passed (its event)
  EpvModelConst *h_model = nullptr;          // [2], pinned
  hipEvent_t ev_model[2] = {nullptr, nullptr};
  uint32_t model_slot = 0;
  uint32_t *d_parent = nullptr, *d_subtree = nullptr;
  double *d_blen = nullptr;
  unsigned long long *d_counters = nullptr;
  unsigned long long *h_counters = nullptr;  // pinned staging for the sharded counters
  unsigned long long *d_cnt_snap = nullptr;  // the counters as they stood when the batch sweeps began (stream-ordered copy:
  unsigned long long *h_cnt_snap = nullptr;  // the host does not wait for the burn-in to read the accept base)
  double *d_partial[2] = {nullptr, nullptr};  // per-block statistics, tree-reduction ping-pong
  uint64_t partial_cap[2] = {0, 0};   // doubles allocated in d_partial[0], [1]
  unsigned long long *d_sweep_tot = nullptr;  // [sweep][B*16] integer statistics of the batch sweeps
  uint64_t sweep_tot_cap = 0;                 // sweeps allocated
  long long *h_tot = nullptr;                 // pinned staging of epv_run_mcmc_counts' totals (one wait for all it reads)
  uint64_t h_tot_cap = 0;                     // words
  double *d_statscale = nullptr;              // [N] 2^k_b of the fixed-point dwell times (epv_suffstat_kernel)
  std::vector<double> statscale;              // host copy; refreshed when the tree or the genome length changes
  double *d_scale = nullptr;
  double *d_lvl = nullptr;      // level outputs of reduce_blocks_to_tot (all batch sweeps at once)
  uint64_t lvl_cap = 0;
  uint8_t *d_stage = nullptr;   // packed-column staging for the halo exchange (grown on demand)
  uint64_t stage_cap = 0;
  hipEvent_t ev_copy[2] = {nullptr, nullptr};   // epv_copy_columns_async: "slot s of my staging buffer is packed"
  EpvIndepConst *d_indep = nullptr;  // [N] constants of the site-independent model
  // launch shapes of the proposal kernels for the uploaded tree and paths (plan_kernels)
  PhaseShapes shapes;
  // global-memory slabs of the first and the third proposal kernel, allocated when a launch first takes the kernel
  double *d_gpool = nullptr, *d_gpool3 = nullptr;
  uint64_t gpool_cap = 0, gpool3_cap = 0;   // doubles allocated
  double *d_segtab = nullptr;    // [B][4][6] single-segment matrices, refreshed by epv_reset
  uint32_t *d_slabflags = nullptr;
  uint32_t *d_nodetab = nullptr; // shapes.v3.nodetab on the device
  uint32_t phase_parity = 0;     // accept lists are double-buffered by phase parity
  EpvFused F{};                  // per-wave lists of the fused colour phase, allocated on first use
  uint64_t fused_waves = 0;      // waves the lists are allocated for
  double kbar = 0.0;  // mean jumps per (site, branch) of the uploaded paths
  double fwd_alloc_ms = 0.0, fwd_sim_ms = 0.0;   // epv_forward_simulate: device memory management / the simulation itself
  // counters / timing
  uint64_t n_sweeps = 0, tot_overflow = 0, tot_coop = 0;
  bool timing = false;           // events around THIS launch (set per launch from timing_every)
  uint32_t timing_every = 0;     // 0 = off, N = HIP events around every N-th colour-phase launch
  uint64_t timing_seen = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  double timed_ms = 0.0;
  uint64_t timed_launches = 0;
  // the posterior summaries of run_mcmc (the structs above), in the order of the chain (kLayers)
  PavgState pa;
  BeventsState be;
  WstatState ws;
  EpochState ep;
  OriginsState lo;
  DomainsState dm;
  PatternsState pt;
  TurnoverState to;
  CorrState co;
  MixingState mx;
  DmapsState dp;
  TractsState tr;
  // leaf cells whose end state is not data (epv_set_unobserved), allocated while unobs_cells > 0:
  // the layout of epv_unobserved (epv_kernels.h)
  uint32_t *d_unobs = nullptr;
  uint64_t unobs_cells = 0;
  // leaf cells that carry evidence instead of data (epv_set_leaf_evidence), allocated while
  // evidence_cells > 0: the layout of epv_leaf_evidence (epv_kernels.h)
  uint32_t *d_evidence = nullptr;
  uint64_t evidence_cells = 0;
  FixedState fx;
};

namespace {

int fail(epv_ctx *c, int code, const std::string &msg) {
  if (c) c->err = msg;
  return code;
}
#define HIP_TRY(c, call)                                                              \
  do {                                                                                \
    hipError_t e_ = (call);                                                           \
    if (e_ != hipSuccess)                                                             \
      return fail((c), EPV_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

template <class T>
void dfree(T *&p) {
  if (p) { (void)hipFree(p); p = nullptr; }
}

// device scratch that is released on every exit path of an entry point
template <class T>
struct DevTmp {
  T *p = nullptr;
  DevTmp() = default;
  DevTmp(const DevTmp &) = delete;
  DevTmp &operator=(const DevTmp &) = delete;
  ~DevTmp() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t count) { return hipMalloc(&p, count * sizeof(T)); }
  T *release() { T *q = p; p = nullptr; return q; }
};

void fixed_off(epv_ctx *c) {
  dfree(c->fx.d_sites); dfree(c->fx.save.sel); dfree(c->fx.save.tri);
  c->fx = FixedState();
}

void free_paths(epv_ctx *c) {
  dfree(c->S.meta); dfree(c->S.jumps); dfree(c->S.sel); dfree(c->S.tri);
  dfree(c->S.prop_llr); dfree(c->S.prop_flag); dfree(c->S.prop_states); dfree(c->S.tasks); dfree(c->S.alist);
  dfree(c->S.segs); dfree(c->S.segout); dfree(c->S.btasks); dfree(c->S.bfirst);
  dfree(c->F.segs); dfree(c->F.outs); dfree(c->F.bt); dfree(c->F.bfirst);
  c->fused_waves = 0;
  dfree(c->d_partial[0]); dfree(c->d_partial[1]);
  c->partial_cap[0] = c->partial_cap[1] = 0;
  dfree(c->d_unobs);   // new paths are new data
  c->unobs_cells = 0;
  dfree(c->d_evidence);
  c->evidence_cells = 0;
  fixed_off(c);
  c->have_paths = c->have_reset = false;
}

int ensure_stage(epv_ctx *c, uint64_t bytes) {
  if (bytes <= c->stage_cap) return EPV_OK;
  dfree(c->d_stage);
  c->stage_cap = 0;
  HIP_TRY(c, hipMalloc(&c->d_stage, bytes));
  c->stage_cap = bytes;
  return EPV_OK;
}

// the launch shapes of every proposal kernel, for the current tree, paths and capacity: decided by plan_shapes
// (epv_plan.h) and kept in the context; the node table of a taken V3 plan goes to the device
int plan_kernels(epv_ctx *c) {
  PhaseShapes shapes = plan_shapes({c->S.N, c->parent.data(), c->subtree.data(), c->S.C, c->S.n, c->kbar}, c->knobs);
  if (shapes.error) return fail(c, EPV_ERR_ARG, shapes.error);
  c->shapes = std::move(shapes);
  PlanV3 &v3 = c->shapes.v3;
  if (!v3.taken) return EPV_OK;
  v3.taken = false;       // (until its table is on the device: a HIP error below leaves the first kernels planned)
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->d_nodetab) HIP_TRY(c, hipMalloc(&c->d_nodetab, 2048u * sizeof(uint32_t)));
  if (!c->d_slabflags) {
    HIP_TRY(c, hipMalloc(&c->d_slabflags, 8u * 256u * sizeof(uint32_t)));
    HIP_TRY(c, hipMemset(c->d_slabflags, 0, 8u * 256u * sizeof(uint32_t)));
  }
  HIP_TRY(c, hipMemcpy(c->d_nodetab, v3.nodetab.data(), v3.nodetab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  v3.taken = true;
  return EPV_OK;
}
PhasePlan phase_plan(const epv_ctx *c) {
  return ::phase_plan(c->shapes, c->knobs, c->S.flags, c->unobs_cells, c->evidence_cells, c->S.B, c->kbar);
}

// per-wave lists of the fused phase, on first use
int ensure_fused_buffers(epv_ctx *c) {
  const uint64_t waves = (c->S.phase_cap + c->shapes.v2.fused_lanes - 1u) / c->shapes.v2.fused_lanes + 4u;
  const uint64_t seg_cap = epv_fused_seg_cap(c->S.B, c->S.C), bt_cap = epv_fused_bt_cap(c->S.B);
  if (c->F.segs && c->fused_waves >= waves && c->F.seg_cap == seg_cap && c->F.bt_cap == bt_cap) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->F.segs); dfree(c->F.outs); dfree(c->F.bt); dfree(c->F.bfirst);
  c->fused_waves = 0;
  HIP_TRY(c, hipMalloc(&c->F.segs, waves * seg_cap * sizeof(EpvSegTask)));
  HIP_TRY(c, hipMalloc(&c->F.outs, waves * seg_cap * sizeof(EpvSegOut)));
  HIP_TRY(c, hipMalloc(&c->F.bt, waves * bt_cap * sizeof(unsigned long long)));
  HIP_TRY(c, hipMalloc(&c->F.bfirst, waves * bt_cap * sizeof(uint32_t)));
  c->F.seg_cap = (uint32_t)seg_cap;
  c->F.bt_cap = (uint32_t)bt_cap;
  c->fused_waves = waves;
  return EPV_OK;
}

// lists of the segment-parallel jump kernels, on first use
int ensure_seg_buffers(epv_ctx *c) {
  if (c->S.segs) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t btask_cap = c->S.task_cap;
  const uint64_t seg_cap = (uint64_t)((double)c->S.task_cap * std::min(8.0, std::max(0.5, 0.5 + 3.0 * c->kbar))) + 256u;
  HIP_TRY(c, hipMalloc(&c->S.segs, seg_cap * EPV_SHARDS * sizeof(EpvSegTask)));
  HIP_TRY(c, hipMalloc(&c->S.segout, seg_cap * EPV_SHARDS * sizeof(EpvSegOut)));
  HIP_TRY(c, hipMalloc(&c->S.btasks, btask_cap * EPV_SHARDS * sizeof(unsigned long long)));
  HIP_TRY(c, hipMalloc(&c->S.bfirst, btask_cap * EPV_SHARDS * sizeof(uint32_t)));
  c->S.btask_cap = btask_cap;
  c->S.seg_cap = seg_cap;
  return EPV_OK;
}

int ensure_partial_doubles(epv_ctx *c, uint64_t need0, uint64_t need1) {
  if (c->partial_cap[0] >= need0 && c->partial_cap[1] >= need1) return EPV_OK;
  need0 = std::max(need0, c->partial_cap[0]);
  need1 = std::max(need1, c->partial_cap[1]);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->d_partial[0]); dfree(c->d_partial[1]);
  c->partial_cap[0] = c->partial_cap[1] = 0;
  HIP_TRY(c, hipMalloc(&c->d_partial[0], need0 * sizeof(double)));
  HIP_TRY(c, hipMalloc(&c->d_partial[1], need1 * sizeof(double)));
  c->partial_cap[0] = need0;
  c->partial_cap[1] = need1;
  return EPV_OK;
}
int ensure_partials(epv_ctx *c, uint64_t nb_min = 0) {
  const uint64_t nb = std::max<uint64_t>((c->S.n + 255u) / 256u, nb_min);
  const uint64_t V = (uint64_t)c->S.B * 16u;
  return ensure_partial_doubles(c, nb * V, ((nb + 255u) / 256u) * V);
}

// Range of local sites a colour phase may update, and the owned range that statistics
// and the accept counter cover.  In halo mode every phase since the last refresh makes
// two more columns at each shard-internal edge stale (their own neighbours were not
// available), so the updatable range shrinks by 2 per phase; the halo must be wide
// enough that it never reaches the owned columns.
void owned_range(const epv_ctx *c, uint64_t *lo, uint64_t *hi) {
  if (!c->halo_mode) { *lo = c->first; *hi = c->last; return; }
  *lo = c->halo_left ? c->halo_left : 1u;
  *hi = c->halo_right ? c->S.n - c->halo_right - 1u : c->S.n - 2u;
}
int phase_range(epv_ctx *c, uint64_t *lo, uint64_t *hi) {
  if (!c->halo_mode) { *lo = c->first; *hi = c->last; return EPV_OK; }
  const uint64_t shrink = 2u * (c->phases_used + 1u);
  *lo = c->halo_left ? shrink : 1u;
  *hi = c->halo_right ? c->S.n - 1u - shrink : c->S.n - 2u;
  if ((c->halo_left && *lo > c->halo_left) || (c->halo_right && *hi + c->halo_right < c->S.n - 1u))
    return fail(c, EPV_ERR_STATE, "halo exhausted: refresh the halo columns (epv_put_columns + "
                                  "epv_set_halo) before running more sweeps");
  return EPV_OK;
}

// ---- exact statistics.  The dwell times of branch b are summed as integers rint(dt * 2^k_b),
//   k_b = min(61 - e(n_global * T_b), 50 - e(T_b)),   e(x) = the frexp exponent (x < 2^e):
// a whole genome's sum stays below 2^61, a single term below 2^50 (epv_stat_fix rounds with one
// add).  oracle/epv_oracle.c (stat_scale_exp) makes the same choice independently.
int stat_scale_exp(uint64_t n_global, double T) {
  if (!(T > 0.0) || !std::isfinite(T)) return 0;
  int e_t = 0, e_nt = 0;
  (void)std::frexp(T, &e_t);
  (void)std::frexp((double)n_global * T, &e_nt);
  int k = std::min(61 - e_nt, 50 - e_t);
  return std::max(-1000, std::min(1000, k));
}
// 2^k_b of every branch on the device, refreshed when the branch lengths or the genome length changed
int ensure_stat_scale(epv_ctx *c) {
  std::vector<double> sc(c->S.N, 1.0);
  for (uint32_t b = 1; b < c->S.N; ++b) sc[b] = std::ldexp(1.0, stat_scale_exp(c->S.n_global, c->blen[b]));
  if (sc == c->statscale) return EPV_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(c->d_statscale, sc.data(), sizeof(double) * c->S.N, hipMemcpyHostToDevice));
  c->statscale = sc;
  return EPV_OK;
}
int ensure_sweep_tot(epv_ctx *c, uint64_t sweeps) {
  if (sweeps <= c->sweep_tot_cap) return EPV_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->d_sweep_tot);
  c->sweep_tot_cap = 0;
  HIP_TRY(c, hipMalloc(&c->d_sweep_tot, sweeps * c->S.B * 16u * sizeof(unsigned long long)));
  c->sweep_tot_cap = sweeps;
  return EPV_OK;
}
void launch_isum(epv_ctx *c, const void *in, uint64_t m, uint64_t G, uint64_t in_row_stride, uint64_t in_z_stride,
                 void *out, uint64_t out_row_stride, uint64_t out_z_stride, uint64_t n_out_rows, uint64_t Z) {
  const uint32_t V = c->S.B * 16u;
  hipLaunchKernelGGL(epv_isum_kernel, dim3(V / 16u, (unsigned)n_out_rows, (unsigned)Z), dim3(256), 0, c->stream,
                     (const unsigned long long *)in, m, V, G, in_row_stride, in_z_stride, (unsigned long long *)out,
                     out_row_stride, out_z_stride);
}
// integer J/D of nb_total blocks x Z slices ([z][block][V] at d_blocks) -> d_sweep_tot[slot0 + z][V]
int reduce_blocks_to_tot(epv_ctx *c, const void *d_blocks, uint64_t nb_total, uint64_t Z, uint64_t slot0) {
  const uint32_t V = c->S.B * 16u;
  int rc = ensure_sweep_tot(c, slot0 + Z);
  if (rc) return rc;
  if (Z > 65535u) return fail(c, EPV_ERR_ARG, "too many batch sweeps for one launch");
  unsigned long long *out = c->d_sweep_tot + slot0 * V;
  if (nb_total <= 1024u) {
    launch_isum(c, d_blocks, nb_total, 0u, V, nb_total * V, out, 0u, V, 1u, Z);
  } else {
    // two stages: groups of 64 blocks (wide grid), then their sums
    const uint64_t m1 = (nb_total + 63u) / 64u;
    if (m1 > 65535u) return fail(c, EPV_ERR_ARG, "more than 2^22 blocks per context");
    if (Z * m1 * V > c->lvl_cap) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      dfree(c->d_lvl);
      c->lvl_cap = 0;
      HIP_TRY(c, hipMalloc(&c->d_lvl, Z * m1 * V * sizeof(double)));
      c->lvl_cap = Z * m1 * V;
    }
    launch_isum(c, d_blocks, nb_total, 64u, V, nb_total * V, c->d_lvl, V, m1 * V, m1, Z);
    launch_isum(c, c->d_lvl, m1, 0u, V, m1 * V, out, 0u, V, 1u, Z);
  }
  HIP_TRY(c, hipGetLastError());
  return EPV_OK;
}
// the integer totals of `batch` sweeps (d_sweep_tot[0 .. batch)) -> tot[batch][B*16] on the host
int read_sweep_tot(epv_ctx *c, uint64_t batch, int64_t *tot) {
  HIP_TRY(c, hipMemcpyAsync(tot, c->d_sweep_tot, batch * c->S.B * 16u * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}
// integer totals tot[batch][B*16] -> J, D as run_mcmc returns them (SingleSiteSampler.cpp:576-594):
// every sweep's statistics become doubles -- J = the count, D = the integer * 2^-k_b, exact but for
// the one rounding of int64 -> double -- and are added up sweep by sweep in fp64 like
// J_all_sites += J_one_site, then divided by the batch size
void counts_to_stats(const epv_ctx *c, const int64_t *tot, uint64_t batch, int average, double *J, double *D) {
  const uint32_t V = c->S.B * 16u;
  const double nb = average ? (double)batch : 1.0;
  for (uint32_t b = 0; b < c->S.B; ++b) {
    const double inv = 1.0 / c->statscale[b + 1u];     // a power of two: exact
    for (int k = 0; k < 8; ++k) {
      double aj = 0.0, ad = 0.0;
      for (uint64_t w = 0; w < batch; ++w) {
        aj += (double)tot[w * V + b * 16u + k];
        ad += (double)tot[w * V + b * 16u + 8u + k] * inv;
      }
      J[b * 8 + k] = aj / nb;
      D[b * 8 + k] = ad / nb;
    }
  }
}
int finish_stats(epv_ctx *c, uint64_t batch, int average, double *J, double *D) {
  std::vector<int64_t> tot(batch * c->S.B * 16u);
  const int rc = read_sweep_tot(c, batch, tot.data());
  if (rc) return rc;
  counts_to_stats(c, tot.data(), batch, average, J, D);
  return EPV_OK;
}

// the triples centred at fixed sites of the owned range, taken off the integer words at `tot` ([B][16]): a fixed site
// is no centre (epv_regions.h).  Nothing is launched while no site is fixed
void launch_fixed_unstat(epv_ctx *c, uint64_t own_lo, uint64_t own_hi, unsigned long long *tot) {
  const uint64_t count = c->fx.off[3];
  if (!count) return;
  hipLaunchKernelGGL(epv_fixed_unstat_kernel, dim3((unsigned)((count * c->S.B + 63u) / 64u)), dim3(64), 0, c->stream, c->S,
                     c->fx.d_sites, count, own_lo, own_hi, c->d_statscale, tot);
}

// integer J/D of the current paths over the owned range into d_sweep_tot[slot]
int launch_suffstats(epv_ctx *c, uint64_t slot) {
  int rc = ensure_partials(c);
  if (rc) return rc;
  if ((rc = ensure_stat_scale(c))) return rc;
  const uint64_t nb = (c->S.n + 255u) / 256u;
  uint64_t own_lo = 0, own_hi = 0;
  owned_range(c, &own_lo, &own_hi);
  hipLaunchKernelGGL(epv_suffstat_kernel, dim3((unsigned)nb, (c->S.B + EPV_STAT_BCH - 1u) / EPV_STAT_BCH), dim3(256), 0,
                     c->stream, c->S, own_lo, own_hi, (uint64_t)0, c->d_statscale, (unsigned long long *)c->d_partial[0]);
  if ((rc = reduce_blocks_to_tot(c, c->d_partial[0], nb, 1u, slot))) return rc;
  launch_fixed_unstat(c, own_lo, own_hi, c->d_sweep_tot + slot * c->S.B * 16u);
  return EPV_OK;
}

// ---- the posterior summaries of run_mcmc ("layers").  What the chain, the destructor and
// the entry points need of a layer, whichever it is; its range, sizes, cap rule, launch and read-out stay its own
struct Layer {
  bool (*on)(const epv_ctx *);
  int (*ensure)(epv_ctx *);                    // (on) the layout fits the sites, tree and scales of now
  int (*check_cap)(epv_ctx *, uint64_t more);  // (on, ensured) `more` further samples fit
  int (*launch)(epv_ctx *);                    // (on, ensured) the resident paths as one sample
  void (*off)(epv_ctx *);                      // no buffers, no layout, no samples
  int (*begin)(epv_ctx *);                     // (on, ensured; may be null) the state after burn-in, before the first
                                               // batch sweep of run_mcmc: for a layer that is joint across samples
  const char *off_msg;                         // what an entry point that needs the layer says while it is off
  const char *name;                            // as the sites-changed failure calls it
};
extern const Layer kPavg, kBevents, kWstat, kEpochs, kOrigins, kDomains, kPatterns, kTurnover, kCorr, kMixing, kDmaps, kTracts;   // (each behind its functions)

int sites_changed(epv_ctx *c, const Layer &L, const char *setter) {
  return fail(c, EPV_ERR_STATE, std::string("the sites of this context changed after ") + L.name + " took samples: " +
                                setter + " again");
}
// (re)lay a layer out with its alloc function.  Whatever fails on the way (not enough memory, a HIP error) leaves
// the layer off: never a layer that is on without its accumulator
int relayout(epv_ctx *c, const Layer &L, int (*alloc)(epv_ctx *)) {
  const int rc = alloc(c);
  if (rc) L.off(c);
  return rc;
}
// the free device memory, and whether `need` bytes fit it with a margin for the read-outs and the kernels' own needs
int device_room(epv_ctx *c, double need, bool *fits, double *free_bytes) {
  size_t free_b = 0, total_b = 0;
  HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
  *fits = !(need + 256.0 * 1024 * 1024 > (double)free_b);
  *free_bytes = (double)free_b;
  return EPV_OK;
}
// `more` further samples fit 32-bit counts that hold `samples` (the branch events and the lineage origins: a site
// adds at most 1024 per sample).  One more that does not fit (a launch) and a batch that would pass the cap
// (refused before the chain) have their own texts
int check_cap32(epv_ctx *c, uint64_t samples, uint64_t more, const char *who, const char *reset) {
  if (samples <= EPV_BEV_MAX_SAMPLES && more <= EPV_BEV_MAX_SAMPLES - samples) return EPV_OK;
  return fail(c, EPV_ERR_STATE, std::string(who) + (more == 1u ? " hold" : " would pass") +
                                " 2^21 samples, the most their 32-bit counts take: read them out and " + reset);
}
// read-out staging of at least `bytes`
template <class T>
int grow_staging(epv_ctx *c, T **buf, uint64_t *cap, uint64_t bytes) {
  if (bytes <= *cap) return EPV_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(*buf);
  *cap = 0;
  HIP_TRY(c, hipMalloc(buf, bytes));
  *cap = bytes;
  return EPV_OK;
}

// The two site ranges a layer counts.  owned_range: the centres of the triples the statistics kernels take.
// pavg_range: a context's owned sites, and the genome's two end sites when it holds them (the sampler never
// changes those, so owned_range leaves them out): over all contexts and GPUs every site is counted once.
void pavg_range(const epv_ctx *c, uint64_t *lo, uint64_t *cnt) {
  uint64_t a = 0, b = 0;
  owned_range(c, &a, &b);
  if (a == 1u && c->S.g0 == 0u) a = 0u;
  if (b + 2u == c->S.n && c->S.g0 + c->S.n == c->S.n_global) b = c->S.n - 1u;
  *lo = a;
  *cnt = b >= a ? b - a + 1u : 0u;
}
// the current layout of either range; the genome's length and B only for a layer that depends on them
SiteLayout owned_layout(const epv_ctx *c) {
  SiteLayout s;
  owned_range(c, &s.lo, &s.hi);
  s.n = c->S.n;
  s.g0 = c->S.g0;
  s.ng = c->S.n_global;
  s.B = c->S.B;
  return s;
}
SiteLayout pavg_layout(const epv_ctx *c, bool with_ng, bool with_B) {
  SiteLayout s;
  pavg_range(c, &s.lo, &s.cnt);
  s.n = c->S.n;
  s.g0 = c->S.g0;
  if (with_ng) s.ng = c->S.n_global;
  if (with_B) s.B = c->S.B;
  return s;
}

// ---- path average (epv_pavg.h): the sites of pavg_range
bool pavg_on(const epv_ctx *c) { return c->pa.P != 0u; }
void pavg_off(epv_ctx *c) {
  dfree(c->pa.d); dfree(c->pa.d_grid); dfree(c->pa.d_out);
  c->pa = PavgState{};
}
// (re)lay out the counts for the current site range; zeroes them
int pavg_alloc(epv_ctx *c) {
  const SiteLayout at = pavg_layout(c, false, true);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->pa.d);
  const double need = 4.0 * (double)c->S.B * (double)at.cnt * (double)c->pa.P;
  bool fits = false;
  double free_b = 0.0;
  const int rc = device_room(c, need, &fits, &free_b);
  if (rc) return rc;
  if (!fits) {
    char buf[320];
    std::snprintf(buf, sizeof buf, "path average of %u points needs %.3g GB of device memory (4 B x %u branches x "
                  "%llu sites x %u points); %.3g GB are free: use fewer points or more GPUs (averaging is off)",
                  c->pa.P, need / 1e9, c->S.B, (unsigned long long)at.cnt, c->pa.P, free_b / 1e9);
    return fail(c, EPV_ERR_ARG, buf);
  }
  const size_t bytes = (size_t)4u * c->S.B * at.cnt * c->pa.P;
  if (bytes) {
    HIP_TRY(c, hipMalloc(&c->pa.d, bytes));
    HIP_TRY(c, hipMemsetAsync(c->pa.d, 0, bytes, c->stream));
  }
  c->pa.at = at;
  c->pa.samples = 0;
  c->pa.grid_blen.clear();
  return EPV_OK;
}
// the counts match the current site range, the grid the current branch lengths
int ensure_pavg(epv_ctx *c) {
  if (!(pavg_layout(c, false, true) == c->pa.at)) {
    if (c->pa.samples) return sites_changed(c, kPavg, "epv_set_path_average");
    const int rc = relayout(c, kPavg, pavg_alloc);
    if (rc) return rc;
  }
  if (c->pa.grid_blen == c->blen) return EPV_OK;
  const uint32_t P = c->pa.P, B = c->S.B;
  std::vector<double> g((size_t)B * P);
  for (uint32_t b = 0; b < B; ++b) {   // average_paths.cpp:33-42: t_1 = bin, t_{i+1} = t_i + bin
    const double bin = c->blen[b + 1u] / (double)(P - 1u);
    double t = bin;
    g[(size_t)b * P] = 0.0;
    for (uint32_t i = 1; i < P; ++i, t += bin) g[(size_t)b * P + i] = t;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (c->pa.grid_blen.empty()) {   // (pavg_alloc: new layout)
    dfree(c->pa.d_grid);
    HIP_TRY(c, hipMalloc(&c->pa.d_grid, g.size() * sizeof(double)));
  }
  HIP_TRY(c, hipMemcpy(c->pa.d_grid, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice));
  c->pa.grid_blen = c->blen;
  return EPV_OK;
}
int pavg_check_cap(epv_ctx *, uint64_t) { return EPV_OK; }   // (no cap is kept: a count takes at most one per sample)
// the resident paths as one sample (ensure_pavg first)
int launch_pavg(epv_ctx *c) {
  if (c->pa.at.cnt)
    hipLaunchKernelGGL(epv_pavg_accum_kernel, dim3((unsigned)((c->pa.at.cnt + 255u) / 256u), c->S.B), dim3(256), 0,
                       c->stream, c->S, c->pa.at.lo, c->pa.at.cnt, (const double *)c->pa.d_grid, c->pa.P, c->pa.d);
  ++c->pa.samples;
  HIP_TRY(c, hipGetLastError());
  return EPV_OK;
}
const Layer kPavg = {pavg_on, ensure_pavg, pavg_check_cap, launch_pavg, pavg_off, nullptr,
                     "path average is off: epv_set_path_average first", "the path average"};

// ---- posterior branch-event maps (epv_bevents.h): the sites of pavg_range, six uint32 planes
bool bevents_on(const epv_ctx *c) { return c->be.on; }
void bevents_off(epv_ctx *c) {
  dfree(c->be.d); dfree(c->be.d_out);
  c->be = BeventsState{};
}
// (re)lay out the planes for the current site range; zeroes them
int bevents_alloc(epv_ctx *c) {
  const SiteLayout at = pavg_layout(c, true, true);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->be.d);
  const double need = 4.0 * EPV_BEV_PLANES * (double)c->S.B * (double)at.cnt;
  bool fits = false;
  double free_b = 0.0;
  const int rc = device_room(c, need, &fits, &free_b);
  if (rc) return rc;
  if (!fits) {
    char buf[320];
    std::snprintf(buf, sizeof buf, "branch events need %.3g GB of device memory (24 B x %u branches x %llu sites); "
                  "%.3g GB are free: use more GPUs (the counters are off)",
                  need / 1e9, c->S.B, (unsigned long long)at.cnt, free_b / 1e9);
    return fail(c, EPV_ERR_ARG, buf);
  }
  const size_t bytes = (size_t)4u * EPV_BEV_PLANES * c->S.B * at.cnt;
  if (bytes) {
    HIP_TRY(c, hipMalloc(&c->be.d, bytes));
    HIP_TRY(c, hipMemsetAsync(c->be.d, 0, bytes, c->stream));
  }
  c->be.at = at;
  c->be.samples = 0;
  return EPV_OK;
}
// the planes match the current site range (there is no grid: branch lengths do not matter)
int ensure_bevents(epv_ctx *c) {
  if (pavg_layout(c, true, true) == c->be.at) return EPV_OK;
  if (c->be.samples) return sites_changed(c, kBevents, "epv_set_branch_events");
  return relayout(c, kBevents, bevents_alloc);
}
int bevents_check_cap(epv_ctx *c, uint64_t more) {
  return check_cap32(c, c->be.samples, more, "branch events", "epv_reset_branch_events");
}
// the resident paths as one sample (ensure_bevents first)
int launch_bevents(epv_ctx *c) {
  const int rc = bevents_check_cap(c, 1u);
  if (rc) return rc;
  if (c->be.at.cnt)
    hipLaunchKernelGGL(epv_bevents_accum_kernel, dim3((unsigned)((c->be.at.cnt + 255u) / 256u)), dim3(256), 0, c->stream,
                       c->S, c->be.at.lo, c->be.at.cnt, c->be.d);
  ++c->be.samples;
  HIP_TRY(c, hipGetLastError());
  return EPV_OK;
}
const Layer kBevents = {bevents_on, ensure_bevents, bevents_check_cap, launch_bevents, bevents_off, nullptr,
                        "branch events are off: epv_set_branch_events first", "the branch events"};

// ---- regional sufficient statistics (epv_wstat.h): J and D per window of W global sites, over the
// triples centred at the sites of owned_range (the statistics kernels' range, not pavg_range: the
// genome's end sites centre no triple)
bool wstat_on(const epv_ctx *c) { return c->ws.W != 0u; }
void wstat_off(epv_ctx *c) {
  dfree(c->ws.d);
  c->ws = WstatState{};
}
// (re)lay out the accumulator for the current site range; zeroes it
int wstat_alloc(epv_ctx *c) {
  const SiteLayout at = owned_layout(c);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->ws.d);
  c->ws.W = std::max<uint64_t>(1u, std::min<uint64_t>(c->ws.W_asked, c->S.n_global));
  const bool any = at.hi >= at.lo && c->S.n >= 3u;
  const uint64_t w0 = any ? (c->S.g0 + at.lo) / c->ws.W : 0u, nw = any ? (c->S.g0 + at.hi) / c->ws.W - w0 + 1u : 0u;
  const double need = 128.0 * (double)c->S.B * (double)nw;
  bool fits = false;
  double free_b = 0.0;
  const int rc = device_room(c, need, &fits, &free_b);
  if (rc) return rc;
  if (!fits) {
    char buf[320];
    std::snprintf(buf, sizeof buf, "window statistics need %.3g GB of device memory (128 B x %u branches x %llu windows "
                  "of %llu sites); %.3g GB are free: use wider windows or more GPUs (the statistics are off)",
                  need / 1e9, c->S.B, (unsigned long long)nw, (unsigned long long)c->ws.W, free_b / 1e9);
    return fail(c, EPV_ERR_ARG, buf);
  }
  const size_t bytes = (size_t)128u * c->S.B * nw;
  if (bytes) {
    HIP_TRY(c, hipMalloc(&c->ws.d, bytes));
    HIP_TRY(c, hipMemsetAsync(c->ws.d, 0, bytes, c->stream));
  }
  c->ws.w0 = w0;
  c->ws.nw = nw;
  c->ws.at = at;
  c->ws.samples = 0;
  c->ws.scale.clear();
  return EPV_OK;
}
// the accumulator matches the current site range, and the scales 2^k_b are the ones its integers were taken with
int ensure_wstat(epv_ctx *c) {
  if (!(owned_layout(c) == c->ws.at)) {
    if (c->ws.samples) return sites_changed(c, kWstat, "epv_set_window_stats");
    const int rc = relayout(c, kWstat, wstat_alloc);
    if (rc) return rc;
  }
  const int rc = ensure_stat_scale(c);
  if (rc) return rc;
  if (c->ws.samples && c->ws.scale != c->statscale)
    return fail(c, EPV_ERR_STATE, "the branch lengths or the genome length changed after the window statistics took "
                                  "samples, so their fixed-point scales 2^k_b differ: read them out and "
                                  "epv_reset_window_stats");
  return EPV_OK;
}
// the most samples the 64-bit sums take: a site adds at most q_b = rint(T_b 2^k_b) + 3072 to a branch's D
// per sample (half a quantum of rounding for each of at most 3 * 2047 + 1 intervals), a window holds at
// most min(W, counted sites) sites: samples * sites * max_b q_b stays below 2^63
uint64_t wstat_max_samples(const epv_ctx *c) {
  uint64_t q = 0;   // (T_b 2^k_b < 2^50: exact in a double and in 64 bits)
  for (uint32_t b = 1; b < c->S.N; ++b)
    q = std::max<uint64_t>(q, (uint64_t)std::llrint(c->blen[b] * c->statscale[b]) + 3072u);
  const uint64_t cnt = c->ws.at.hi >= c->ws.at.lo ? c->ws.at.hi - c->ws.at.lo + 1u : 0u;
  const unsigned __int128 per = (unsigned __int128)std::min<uint64_t>(c->ws.W, cnt) * q;
  if (!per) return UINT64_MAX;
  return (uint64_t)((((unsigned __int128)1 << 63) - 1u) / per);   // the most m with m * per < 2^63
}
// `batch` more samples fit (ensure_wstat first)
int wstat_check_cap(epv_ctx *c, uint64_t batch) {
  const uint64_t most = wstat_max_samples(c);
  if (c->ws.samples > most || batch > most - c->ws.samples) {
    char buf[320];
    std::snprintf(buf, sizeof buf, "window statistics with windows of %llu sites take at most %llu samples in their "
                  "64-bit sums and hold %llu: read them out and epv_reset_window_stats",
                  (unsigned long long)c->ws.W, (unsigned long long)most, (unsigned long long)c->ws.samples);
    return fail(c, EPV_ERR_STATE, buf);
  }
  return EPV_OK;
}
// the resident paths as one sample (ensure_wstat first)
int launch_wstat(epv_ctx *c) {
  int rc = wstat_check_cap(c, 1u);
  if (rc) return rc;
  if (c->ws.nw) {
    const uint64_t tiles = (c->ws.at.hi - c->ws.at.lo) / 64u + 1u;
    if (tiles > 0x7fffffffull) return fail(c, EPV_ERR_ARG, "too many sites in one context for the window statistics");
    const dim3 grid((unsigned)tiles, (c->S.B + EPV_WSTAT_BCH - 1u) / EPV_WSTAT_BCH);
    if (c->ws.W < 64u)
      hipLaunchKernelGGL(epv_wstat_accum_kernel<true>, grid, dim3(64), 0, c->stream, c->S, c->ws.at.lo, c->ws.at.hi,
                         c->d_statscale, c->ws.W, c->ws.w0, c->ws.nw, c->ws.d);
    else
      hipLaunchKernelGGL(epv_wstat_accum_kernel<false>, grid, dim3(64), 0, c->stream, c->S, c->ws.at.lo, c->ws.at.hi,
                         c->d_statscale, c->ws.W, c->ws.w0, c->ws.nw, c->ws.d);
  }
  HIP_TRY(c, hipGetLastError());
  if (!c->ws.samples) c->ws.scale = c->statscale;
  ++c->ws.samples;
  return EPV_OK;
}
const Layer kWstat = {wstat_on, ensure_wstat, wstat_check_cap, launch_wstat, wstat_off, nullptr,
                      "window statistics are off: epv_set_window_stats first", "the window statistics"};

// ---- lineage origin maps (epv_origin.h): the sites of pavg_range; origin uint32 [R][cnt], age uint64 [L][cnt]
bool origins_on(const epv_ctx *c) { return c->lo.on; }
void origins_off(epv_ctx *c) {
  dfree(c->lo.d); dfree(c->lo.d_age); dfree(c->lo.d_first); dfree(c->lo.d_rowb); dfree(c->lo.d_fixT); dfree(c->lo.d_out);
  c->lo = OriginsState{};
}
// k = 40 - e(H), H = the longest lineage (fp64 sums from the leaf upward), and fixT[v] = llrint(ldexp(T_v, k)):
// an age term stays below 2^40, so 2^21 samples stay below 2^63
void origins_scale(const epv_ctx *c, int *k, std::vector<long long> *fixT) {
  double H = 0.0;
  for (uint32_t v = 1; v < c->S.N; ++v) {
    if (c->subtree[v] != 1u) continue;
    double h = 0.0;
    for (uint32_t u = v; u != 0u; u = c->parent[u]) h += c->blen[u];
    if (!(h <= H)) H = h;   // (a NaN sum stays and gives k = 0)
  }
  *k = 0;
  if (H > 0.0 && std::isfinite(H)) {
    int e = 0;
    (void)std::frexp(H, &e);
    *k = std::max(-1000, std::min(1000, 40 - e));
  }
  fixT->assign(c->S.N, 0);
  for (uint32_t v = 1; v < c->S.N; ++v) (*fixT)[v] = std::llrint(std::ldexp(c->blen[v], *k));
}
// (re)lay out the accumulators and tables for the current tree and site range; zeroes them
int origins_alloc(epv_ctx *c) {
  const SiteLayout at = pavg_layout(c, true, false);
  const uint64_t cnt = at.cnt;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->lo.d); dfree(c->lo.d_age); dfree(c->lo.d_first); dfree(c->lo.d_rowb); dfree(c->lo.d_fixT);
  // the row table: per leaf in node order its lineage from the leaf upward, then the root row
  std::vector<uint32_t> first, leaf, rowb;
  for (uint32_t v = 1; v < c->S.N; ++v) {
    if (c->subtree[v] != 1u) continue;
    first.push_back((uint32_t)rowb.size());
    for (uint32_t u = v; u != 0u; u = c->parent[u]) { leaf.push_back(v); rowb.push_back(u); }
    leaf.push_back(v);
    rowb.push_back(0u);
  }
  const uint32_t L = (uint32_t)first.size(), R = (uint32_t)rowb.size();
  first.push_back(R);
  const double need = (4.0 * R + 8.0 * L) * (double)cnt;
  bool fits = false;
  double free_b = 0.0;
  const int rc = device_room(c, need, &fits, &free_b);
  if (rc) return rc;
  if (!fits) {
    char buf[320];
    std::snprintf(buf, sizeof buf, "lineage origins need %.3g GB of device memory ((4 B x %u rows + 8 B x %u leaves) x "
                  "%llu sites); %.3g GB are free: use more GPUs (the maps are off)",
                  need / 1e9, R, L, (unsigned long long)cnt, free_b / 1e9);
    return fail(c, EPV_ERR_ARG, buf);
  }
  int k = 0;
  std::vector<long long> fixT;
  origins_scale(c, &k, &fixT);
  HIP_TRY(c, hipMalloc(&c->lo.d_first, sizeof(uint32_t) * first.size()));
  HIP_TRY(c, hipMalloc(&c->lo.d_rowb, sizeof(uint32_t) * rowb.size()));
  HIP_TRY(c, hipMalloc(&c->lo.d_fixT, sizeof(long long) * fixT.size()));
  HIP_TRY(c, hipMemcpy(c->lo.d_first, first.data(), sizeof(uint32_t) * first.size(), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->lo.d_rowb, rowb.data(), sizeof(uint32_t) * rowb.size(), hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->lo.d_fixT, fixT.data(), sizeof(long long) * fixT.size(), hipMemcpyHostToDevice));
  if (cnt) {
    HIP_TRY(c, hipMalloc(&c->lo.d, (size_t)4u * R * cnt));
    HIP_TRY(c, hipMalloc(&c->lo.d_age, (size_t)8u * L * cnt));
    HIP_TRY(c, hipMemsetAsync(c->lo.d, 0, (size_t)4u * R * cnt, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->lo.d_age, 0, (size_t)8u * L * cnt, c->stream));
  }
  c->lo.at = at;
  c->lo.L = L;
  c->lo.R = R;
  c->lo.samples = 0;
  c->lo.parent = c->parent;
  c->lo.first.swap(first);
  c->lo.leaf.swap(leaf);
  c->lo.rowb.swap(rowb);
  c->lo.fixT.swap(fixT);
  c->lo.k = k;
  return EPV_OK;
}
// the accumulators match the current site range, and the tree, k and fixT are the ones the samples were taken with
int ensure_origins(epv_ctx *c) {
  const bool sites = !(pavg_layout(c, true, false) == c->lo.at);
  int k = 0;
  std::vector<long long> fixT;
  origins_scale(c, &k, &fixT);
  const bool tree = c->parent != c->lo.parent || k != c->lo.k || fixT != c->lo.fixT;
  if (!sites && !tree) return EPV_OK;
  if (c->lo.samples) {
    if (sites) return sites_changed(c, kOrigins, "epv_set_lineage_origins");
    return fail(c, EPV_ERR_STATE, "the tree or the branch lengths changed after the lineage origins took samples, so "
                                  "their rows or fixed-point ages differ: read them out and epv_reset_lineage_origins");
  }
  return relayout(c, kOrigins, origins_alloc);
}
int origins_check_cap(epv_ctx *c, uint64_t more) {
  return check_cap32(c, c->lo.samples, more, "lineage origins", "epv_reset_lineage_origins");
}
// the resident paths as one sample (ensure_origins first)
int launch_origins(epv_ctx *c) {
  const int rc = origins_check_cap(c, 1u);
  if (rc) return rc;
  if (c->lo.at.cnt && c->lo.L)
    hipLaunchKernelGGL(epv_origin_accum_kernel, dim3((unsigned)((c->lo.at.cnt + 255u) / 256u), c->lo.L), dim3(256), 0,
                       c->stream, c->S, c->lo.at.lo, c->lo.at.cnt, (const uint32_t *)c->lo.d_first,
                       (const uint32_t *)c->lo.d_rowb, (const long long *)c->lo.d_fixT, std::ldexp(1.0, c->lo.k),
                       c->lo.d, c->lo.d_age);
  HIP_TRY(c, hipGetLastError());
  ++c->lo.samples;
  return EPV_OK;
}
const Layer kOrigins = {origins_on, ensure_origins, origins_check_cap, launch_origins, origins_off, nullptr,
                        "lineage origins are off: epv_set_lineage_origins first", "the lineage origins"};

// ---- the summaries that are joint along the genome: the sites of pavg_range; a context
// keeps its PART (PartState), unclosed.  What the five share is here once; a layer adds its describe function, its
// launch and what its entry points take and give
struct PartDesc {
  PartShape shape;              // every size of the part (epv_part.h)
  std::vector<uint32_t> tree;   // what of the tree the rows depend on beyond B: a change of it after samples is refused
  std::string terms;            // the factors of the shape's sizes, for the device-room text
  std::string refusal;          // (not empty) the stretch is too short for the layer: why
};
struct PartKind {
  const Layer &layer;
  const char *noun, *setter, *reset;   // as the texts call the layer, and the entry points they tell to call
  const char *advice;                  // what to do when the part does not fit the device
  bool with_B;                         // the site layout holds B: the rows depend on nothing else of the tree
  PartDesc (*describe)(const epv_ctx *, uint64_t cnt);   // the part of cnt counted sites for the context as it is now
};
std::string text(const char *format, ...) __attribute__((format(printf, 1, 2)));
std::string text(const char *format, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, format);
  std::vsnprintf(buf, sizeof buf, format, ap);
  va_end(ap);
  return buf;
}
// the root's lowest-numbered child: what the root's row is read from
uint32_t corr_child0(const epv_ctx *c) {
  for (uint32_t v = 1; v < c->S.N; ++v) if (c->parent[v] == 0u) return v;
  return 0u;
}
void part_free(PartState &p) { dfree(p.d_acc[0]); dfree(p.d_acc[1]); dfree(p.d_edge); dfree(p.d_bits); }
template <class State>
void part_off(State &s) {
  part_free(s);
  s = State{};
}
// no samples: the accumulators and the edge records zeroed (the scratch is written before it is read)
int part_zero(epv_ctx *c, PartState &p) {
  for (int i = 0; i < 2; ++i)
    if (p.shape.acc_b[i]) HIP_TRY(c, hipMemsetAsync(p.d_acc[i], 0, p.shape.acc_b[i], c->stream));
  if (p.shape.edges_b) HIP_TRY(c, hipMemsetAsync(p.d_edge, 0, p.shape.edges_b, c->stream));
  p.samples = 0;
  return EPV_OK;
}
// (re)lay out the part for the current tree and site range; zeroes it
int part_alloc(epv_ctx *c, const PartKind &K, PartState &p) {
  const SiteLayout at = pavg_layout(c, true, K.with_B);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  part_free(p);
  if (at.cnt >> 32) return fail(c, EPV_ERR_ARG, std::string(K.noun) + ": at most 2^32 - 1 sites per context");
  PartDesc d = K.describe(c, at.cnt);
  if (!d.refusal.empty()) return fail(c, EPV_ERR_ARG, d.refusal);
  const PartShape &sh = d.shape;
  const double need = (double)sh.total();
  bool fits = false;
  double free_b = 0.0;
  const int rc = device_room(c, need, &fits, &free_b);
  if (rc) return rc;
  if (!fits)
    return fail(c, EPV_ERR_ARG, text("%s: %.3g GB of device memory are needed (%s); %.3g GB are free: %s", K.noun,
                                     need / 1e9, d.terms.c_str(), free_b / 1e9, K.advice));
  if (sh.bits_b) HIP_TRY(c, hipMalloc(&p.d_bits, sh.bits_b));
  if (sh.edges_b) HIP_TRY(c, hipMalloc(&p.d_edge, sh.edges_b));
  for (int i = 0; i < 2; ++i)
    if (sh.acc_b[i]) HIP_TRY(c, hipMalloc(&p.d_acc[i], sh.acc_b[i]));
  p.at = at;
  p.shape = sh;
  p.tree.swap(d.tree);
  return part_zero(c, p);
}
// the part matches the current site range and what its rows depend on of the tree (branch lengths never matter: no
// jump time is read)
int part_ensure(epv_ctx *c, const PartKind &K, const PartState &p, int (*alloc)(epv_ctx *)) {
  const SiteLayout at = pavg_layout(c, true, K.with_B);
  const bool sites = !(at == p.at);
  if (!sites && K.describe(c, at.cnt).tree == p.tree) return EPV_OK;
  if (p.samples) {
    if (sites) return sites_changed(c, K.layer, K.setter);
    return fail(c, EPV_ERR_STATE, std::string("the tree changed after ") + K.layer.name + " took samples: read them out and " +
                                  K.reset);
  }
  return relayout(c, K.layer, alloc);
}
// `more` further samples fit the edge records
int part_check_cap(epv_ctx *c, const PartKind &K, const PartState &p, uint64_t more) {
  if (p.samples + more <= p.max) return EPV_OK;
  return fail(c, EPV_ERR_STATE, text("%s: %llu of the %llu samples the edge records were allocated for are held, and "
                                     "%llu more were asked: read them out and %s, or %s with more", K.noun,
                                     (unsigned long long)p.samples, (unsigned long long)p.max, (unsigned long long)more,
                                     K.reset, K.setter));
}
// the resident paths as one sample (the layer's ensure first).  While `counts`: the rows ROWS of epv_rows.h into the
// part's scratch, then one(r0, nr, bits, words, edge) launches the layer's kernel over rows r0 .. r0 + nr - 1 of
// `rows`, at most `slice` at a time (a grid's y dimension takes 65535 rows); edge = this sample's records
template <uint32_t ROWS, class One>
int part_sample(epv_ctx *c, const PartKind &K, PartState &p, bool counts, uint32_t child0, uint32_t state, uint32_t rows,
                uint32_t slice, One one) {
  const int rc = K.layer.check_cap(c, 1u);
  if (rc) return rc;
  if (counts) {
    const uint64_t words = p.shape.words;
    hipLaunchKernelGGL(epv_rows_pack_kernel<ROWS>, dim3((unsigned)((words + 3u) / 4u)), dim3(256), 0, c->stream, c->S, p.at.lo,
                       p.at.cnt, words, child0, state, p.d_bits);
    HIP_TRY(c, hipGetLastError());
    unsigned long long *edge = p.d_edge + p.samples * (p.shape.edge_b / 8u);
    for (uint32_t r0 = 0; r0 < rows; r0 += slice) {
      one(r0, std::min<uint32_t>(slice, rows - r0), (const unsigned long long *)p.d_bits, words, edge);
      HIP_TRY(c, hipGetLastError());
    }
  }
  ++p.samples;
  return EPV_OK;
}
// blocks along a row of `words` words, chunk words a block
unsigned part_chunks(uint64_t words, uint32_t chunk) { return (unsigned)((words + chunk - 1u) / chunk); }

// ---- domain size spectra (epv_domains.h): N node rows; the part depends on the whole tree
PartDesc domains_part(const epv_ctx *c, uint64_t cnt) {
  PartDesc d;
  d.shape = domains_shape(c->S.N, cnt, c->dm.max);
  d.tree = c->parent;
  d.terms = text("16 B x %u nodes x %llu samples of edge records, 8 B x %u nodes x %llu words of node states", c->S.N,
                 (unsigned long long)c->dm.max, c->S.N, (unsigned long long)d.shape.words);
  return d;
}
const PartKind kDomainsPart = {kDomains, "domain statistics", "epv_set_domain_stats", "epv_reset_domain_stats",
                               "ask for fewer samples (the statistics are off)", false, domains_part};
bool domains_on(const epv_ctx *c) { return c->dm.on; }
void domains_off(epv_ctx *c) { part_off(c->dm); }
int domains_alloc(epv_ctx *c) {
  const int rc = part_alloc(c, kDomainsPart, c->dm);
  if (!rc) c->dm.child0 = corr_child0(c);
  return rc;
}
int ensure_domains(epv_ctx *c) { return part_ensure(c, kDomainsPart, c->dm, domains_alloc); }
int domains_check_cap(epv_ctx *c, uint64_t more) { return part_check_cap(c, kDomainsPart, c->dm, more); }
// pack the node states, then count the runs
int launch_domains(epv_ctx *c) {
  DomainsState &p = c->dm;
  return part_sample<EPV_ROWS_NODE>(c, kDomainsPart, p, p.at.cnt != 0u, p.child0, 1u, p.shape.rows, 65535u,
    [&](uint32_t v0, uint32_t nv, const unsigned long long *bits, uint64_t words, unsigned long long *edge) {
      hipLaunchKernelGGL(epv_dom_runs_kernel, dim3(part_chunks(words, EPV_DOM_CHUNK_WORDS), nv), dim3(256), 0, c->stream, bits,
                         words, p.at.cnt, v0, (unsigned long long *)p.d_acc[0], (unsigned long long *)p.d_acc[1], edge);
    });
}
const Layer kDomains = {domains_on, ensure_domains, domains_check_cap, launch_domains, domains_off, nullptr,
                        "domain statistics are off: epv_set_domain_stats first", "the domain statistics"};

// ---- domain turnover (epv_turnover.h): R = 2 B end rows; neither the tree's shape nor its branch lengths matter
PartDesc turnover_part(const epv_ctx *c, uint64_t cnt) {
  PartDesc d;
  d.shape = turnover_shape(c->S.B, cnt, c->to.max);
  d.terms = text("16 B x %u rows x %llu samples of edge records, 8 B x %u rows x %llu words of row states", d.shape.rows,
                 (unsigned long long)c->to.max, d.shape.rows, (unsigned long long)d.shape.words);
  return d;
}
const PartKind kTurnoverPart = {kTurnover, "domain turnover", "epv_set_domain_turnover", "epv_reset_domain_turnover",
                                "ask for fewer samples (the turnover is off)", true, turnover_part};
bool turnover_on(const epv_ctx *c) { return c->to.on; }
void turnover_off(epv_ctx *c) { part_off(c->to); }
int turnover_alloc(epv_ctx *c) { return part_alloc(c, kTurnoverPart, c->to); }
int ensure_turnover(epv_ctx *c) { return part_ensure(c, kTurnoverPart, c->to, turnover_alloc); }
int turnover_check_cap(epv_ctx *c, uint64_t more) { return part_check_cap(c, kTurnoverPart, c->to, more); }
// pack the rows, then count the runs (slices of an even number of rows: a row's partner is in its slice)
int launch_turnover(epv_ctx *c) {
  TurnoverState &p = c->to;
  return part_sample<EPV_ROWS_ENDS>(c, kTurnoverPart, p, p.at.cnt && p.shape.rows, 0u, 1u, p.shape.rows, 65534u,
    [&](uint32_t r0, uint32_t nr, const unsigned long long *bits, uint64_t words, unsigned long long *edge) {
      hipLaunchKernelGGL(epv_turn_runs_kernel, dim3(part_chunks(words, EPV_DOM_CHUNK_WORDS), nr), dim3(256), 0, c->stream, bits,
                         words, p.at.cnt, r0, (unsigned long long *)p.d_acc[0], (unsigned long long *)p.d_acc[1], edge);
    });
}
const Layer kTurnover = {turnover_on, ensure_turnover, turnover_check_cap, launch_turnover, turnover_off, nullptr,
                         "domain turnover is off: epv_set_domain_turnover first", "the domain turnover"};

// ---- spatial correlations (epv_corr.h): R = N + B rows, the node rows and the change rows; of the tree the number
// of nodes and the root's first child matter
PartDesc corr_part(const epv_ctx *c, uint64_t cnt) {
  PartDesc d;
  const uint32_t L = c->co.L, LW = (L + 63u) / 64u;
  d.shape = corr_shape(c->S.N, c->S.B, L, cnt, c->co.max);
  d.tree = {c->S.N, corr_child0(c)};
  d.terms = text("16 B x %u rows x %u words x %llu samples of edge records, 8 B x %u rows x %llu words of row states, "
                 "8 B x %u rows x %u lags of counts", d.shape.rows, LW, (unsigned long long)c->co.max, d.shape.rows,
                 (unsigned long long)d.shape.words, d.shape.rows, L + 1u);
  if (cnt < L)   // (a pair may span two parts, never three)
    d.refusal = text("spatial correlations: this context counts %llu sites, fewer than max_lag = %u: a context's stretch "
                     "holds at least max_lag sites (the correlations are off)", (unsigned long long)cnt, L);
  return d;
}
const PartKind kCorrPart = {kCorr, "spatial correlations", "epv_set_spatial_correlation", "epv_reset_spatial_correlation",
                            "ask for fewer samples (the correlations are off)", true, corr_part};
bool corr_on(const epv_ctx *c) { return c->co.L != 0u; }
void corr_off(epv_ctx *c) { part_off(c->co); }
int corr_alloc(epv_ctx *c) {
  const int rc = part_alloc(c, kCorrPart, c->co);
  if (!rc) c->co.child0 = corr_child0(c);
  return rc;
}
int ensure_corr(epv_ctx *c) { return part_ensure(c, kCorrPart, c->co, corr_alloc); }
int corr_check_cap(epv_ctx *c, uint64_t more) { return part_check_cap(c, kCorrPart, c->co, more); }
// pack the rows, then count the pairs of every lag (no guard: a stretch holds at least max_lag >= 1 sites, and a tree
// at least one branch)
int launch_corr(epv_ctx *c) {
  CorrState &p = c->co;
  const unsigned threads = std::min<unsigned>(256u, (p.L + 1u + 63u) / 64u * 64u);   // (a thread owns lags)
  return part_sample<EPV_ROWS_CORR>(c, kCorrPart, p, true, p.child0, 1u, p.shape.rows, 65535u,
    [&](uint32_t r0, uint32_t nr, const unsigned long long *bits, uint64_t words, unsigned long long *edge) {
      hipLaunchKernelGGL(epv_corr_count_kernel, dim3(part_chunks(words, EPV_CORR_CHUNK_WORDS), nr), dim3(threads), 0, c->stream,
                         bits, words, p.at.cnt, r0, p.L, (unsigned long long *)p.d_acc[0], edge);
    });
}
const Layer kCorr = {corr_on, ensure_corr, corr_check_cap, launch_corr, corr_off, nullptr,
                     "spatial correlations are off: epv_set_spatial_correlation first", "the spatial correlations"};

// ---- change patterns (epv_patterns.h): the sites of pavg_range, R = 12 + 2 B + I uint32 rows
bool patterns_on(const epv_ctx *c) { return c->pt.on; }
void patterns_off(epv_ctx *c) {
  dfree(c->pt.d); dfree(c->pt.d_out);
  c->pt = PatternsState{};
}
// (re)lay out the rows for the current tree and site range; zeroes them
int patterns_alloc(epv_ctx *c) {
  const SiteLayout at = pavg_layout(c, true, true);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->pt.d);
  uint32_t I = 0;
  for (uint32_t v = 1; v < c->S.N; ++v) I += c->subtree[v] > 1u;
  const uint32_t R = EPV_PAT_FIXED + 2u * c->S.B + I;
  const double need = 4.0 * (double)R * (double)at.cnt;
  bool fits = false;
  double free_b = 0.0;
  const int rc = device_room(c, need, &fits, &free_b);
  if (rc) return rc;
  if (!fits) {
    char buf[320];
    std::snprintf(buf, sizeof buf, "change patterns need %.3g GB of device memory (4 B x %u rows x %llu sites); "
                  "%.3g GB are free: use more GPUs (the counters are off)",
                  need / 1e9, R, (unsigned long long)at.cnt, free_b / 1e9);
    return fail(c, EPV_ERR_ARG, buf);
  }
  const size_t bytes = (size_t)4u * R * at.cnt;
  if (bytes) {
    HIP_TRY(c, hipMalloc(&c->pt.d, bytes));
    HIP_TRY(c, hipMemsetAsync(c->pt.d, 0, bytes, c->stream));
  }
  c->pt.at = at;
  c->pt.I = I;
  c->pt.R = R;
  c->pt.samples = 0;
  c->pt.subtree = c->subtree;
  return EPV_OK;
}
// the rows match the current site range and tree (branch lengths do not matter: no jump time is read)
int ensure_patterns(epv_ctx *c) {
  const bool sites = !(pavg_layout(c, true, true) == c->pt.at);
  if (!sites && c->subtree == c->pt.subtree) return EPV_OK;
  if (c->pt.samples) {
    if (sites) return sites_changed(c, kPatterns, "epv_set_change_patterns");
    return fail(c, EPV_ERR_STATE, "the tree changed after the change patterns took samples: read them out and "
                                  "epv_reset_change_patterns");
  }
  return relayout(c, kPatterns, patterns_alloc);
}
int patterns_check_cap(epv_ctx *, uint64_t) { return EPV_OK; }   // (no cap is kept: a count takes at most one per sample)
// the resident paths as one sample (ensure_patterns first)
int launch_patterns(epv_ctx *c) {
  if (c->pt.at.cnt)
    hipLaunchKernelGGL(epv_patterns_accum_kernel, dim3((unsigned)((c->pt.at.cnt + 255u) / 256u)), dim3(256), 0, c->stream,
                       c->S, c->pt.at.lo, c->pt.at.cnt, c->pt.I, c->pt.d);
  ++c->pt.samples;
  HIP_TRY(c, hipGetLastError());
  return EPV_OK;
}
const Layer kPatterns = {patterns_on, ensure_patterns, patterns_check_cap, launch_patterns, patterns_off, nullptr,
                         "change patterns are off: epv_set_change_patterns first", "the change patterns"};

// ---- epoch statistics (epv_epochs.h): J and D per branch and epoch of the branch, over the triples centred
// at the sites of owned_range.  The accumulator [B][P][32] does not depend on the site range
bool epoch_on(const epv_ctx *c) { return c->ep.P != 0u; }
void epoch_off(epv_ctx *c) {
  dfree(c->ep.d);
  c->ep = EpochState{};
}
// (re)lay out the accumulator of ep.P epochs for the current tree; zeroes it
int epoch_alloc(epv_ctx *c) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->ep.d);
  const size_t bytes = (size_t)256u * c->S.B * c->ep.P;
  if (bytes) {
    HIP_TRY(c, hipMalloc(&c->ep.d, bytes));
    HIP_TRY(c, hipMemsetAsync(c->ep.d, 0, bytes, c->stream));
  }
  c->ep.B = c->S.B;
  c->ep.samples = 0;
  c->ep.addends = 0;
  c->ep.scale.clear();
  c->ep.fixT.clear();
  return EPV_OK;
}
// the accumulator matches the current tree, and the scales 2^k_b are the ones its integers were taken with
int ensure_epochs(epv_ctx *c) {
  if (c->S.B != c->ep.B) {
    if (c->ep.samples)
      return fail(c, EPV_ERR_STATE, "the tree of this context changed after the epoch statistics took samples: "
                                    "epv_set_epoch_stats again");
    const int rc = relayout(c, kEpochs, epoch_alloc);
    if (rc) return rc;
  }
  const int rc = ensure_stat_scale(c);
  if (rc) return rc;
  if (c->ep.samples && c->ep.scale != c->statscale)
    return fail(c, EPV_ERR_STATE, "the branch lengths or the genome length changed after the epoch statistics took "
                                  "samples, so their fixed-point scales 2^k_b differ: read them out and "
                                  "epv_reset_epoch_stats");
  return EPV_OK;
}
// 256-site tiles per block of epv_epoch_accum_kernel: about a thousand blocks where the sites allow it (a
// block's flush costs up to 32 P atomics whatever it covered), at most EPV_EPOCH_MAX_TILES
uint32_t epoch_tiles(const epv_ctx *c, uint64_t lo, uint64_t hi) {
  if (hi < lo) return 1u;
  const uint64_t tiles = (hi - lo) / 256u + 1u;
  const uint64_t want = (tiles * std::max<uint32_t>(c->S.B, 1u) + 1023u) / 1024u;
  return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>(want, EPV_EPOCH_MAX_TILES));
}
// blocks along the sites of one launch over the current owned range
uint64_t epoch_blocks(const epv_ctx *c) {
  uint64_t lo = 0, hi = 0;
  owned_range(c, &lo, &hi);
  return hi >= lo ? (hi - lo) / (256ull * epoch_tiles(c, lo, hi)) + 1u : 0u;
}
// `batch` more samples fit (ensure_epochs first): a block adds at most one addend below 2^32 to a global
// word per sample (the lo and hi halves of its 64-bit sum, its counts), so the 64-bit words hold while
//   addends so far + batch * blocks along the sites < 2^32
// (ep.addends counts the blocks of every sample taken, whatever the owned range was then)
int epoch_check_cap(epv_ctx *c, uint64_t batch) {
  const uint64_t blocks = epoch_blocks(c), room = (1ull << 32) - 1u;
  if (!blocks) return EPV_OK;
  const uint64_t left = c->ep.addends > room ? 0u : (room - c->ep.addends) / blocks;   // samples that still fit
  if (c->ep.addends > room || batch > left) {
    char buf[320];
    std::snprintf(buf, sizeof buf, "epoch statistics over %llu blocks of sites take at most %llu samples in their "
                  "64-bit sums and hold %llu: read them out and epv_reset_epoch_stats",
                  (unsigned long long)blocks, (unsigned long long)(c->ep.samples + left), (unsigned long long)c->ep.samples);
    return fail(c, EPV_ERR_STATE, buf);
  }
  return EPV_OK;
}
// the scales and branch lengths of now become the ones the accumulator's integers mean
void epoch_remember(epv_ctx *c) {
  c->ep.scale = c->statscale;
  c->ep.fixT.assign(c->S.N, 0u);
  for (uint32_t b = 1; b < c->S.N; ++b) c->ep.fixT[b] = (uint64_t)std::llrint(c->blen[b] * c->statscale[b]);   // (< 2^50: exact)
}
// the resident paths as one sample (ensure_epochs first)
int launch_epochs(epv_ctx *c) {
  int rc = epoch_check_cap(c, 1u);
  if (rc) return rc;
  uint64_t lo = 0, hi = 0;
  owned_range(c, &lo, &hi);
  if (hi >= lo && c->S.n >= 3u && c->S.B) {
    const uint32_t tiles = epoch_tiles(c, lo, hi);
    const uint64_t blocks = (hi - lo) / (256ull * tiles) + 1u;
    if (blocks > 0x7fffffffull) return fail(c, EPV_ERR_ARG, "too many sites in one context for the epoch statistics");
    hipLaunchKernelGGL(epv_epoch_accum_kernel, dim3((unsigned)blocks, c->S.B), dim3(256), (size_t)136u * c->ep.P,
                       c->stream, c->S, lo, hi, c->d_statscale, c->ep.P, tiles, c->ep.d);
  }
  HIP_TRY(c, hipGetLastError());
  if (!c->ep.samples) epoch_remember(c);
  ++c->ep.samples;
  c->ep.addends += epoch_blocks(c);
  return EPV_OK;
}
const Layer kEpochs = {epoch_on, ensure_epochs, epoch_check_cap, launch_epochs, epoch_off, nullptr,
                       "epoch statistics are off: epv_set_epoch_stats first", "the epoch statistics"};

// ---- chain mixing diagnostics (epv_mixing.h): the sites of pavg_range; per site a fingerprint, a move count,
// 2 + K sums and a ring of K jump counts.  The host keeps the run: which sample is linked to which
bool mixing_on(const epv_ctx *c) { return c->mx.K != 0u; }
void mixing_off(epv_ctx *c) {
  dfree(c->mx.d_fp); dfree(c->mx.d_moved); dfree(c->mx.d_sums); dfree(c->mx.d_ring); dfree(c->mx.d_out);
  c->mx = MixingState{};
}
// no sample is linked to the one before it until a run opens again
void mixing_close_run(epv_ctx *c) {
  c->mx.run_open = false;
  c->mx.run_len = 0;
}
// no samples, no run: the accumulators zeroed (the fingerprints and the ring are written before they are read)
int mixing_zero(epv_ctx *c) {
  const uint64_t cnt = c->mx.at.cnt, K = c->mx.K;
  if (cnt) {
    HIP_TRY(c, hipMemsetAsync(c->mx.d_fp, 0, 8u * cnt, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->mx.d_moved, 0, 4u * cnt, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->mx.d_sums, 0, 8u * (2u + K) * cnt, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->mx.d_ring, 0, 4u * K * cnt, c->stream));
  }
  c->mx.samples = c->mx.moved_pairs = 0;
  for (uint64_t &p : c->mx.pairs) p = 0;
  mixing_close_run(c);
  return EPV_OK;
}
// (re)lay out the buffers for the current site range; zeroes them
int mixing_alloc(epv_ctx *c) {
  const SiteLayout at = pavg_layout(c, true, true);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(c->mx.d_fp); dfree(c->mx.d_moved); dfree(c->mx.d_sums); dfree(c->mx.d_ring);
  const uint32_t K = c->mx.K, per_site = 28u + 12u * K;
  const double need = (double)per_site * (double)at.cnt;
  bool fits = false;
  double free_b = 0.0;
  const int rc = device_room(c, need, &fits, &free_b);
  if (rc) return rc;
  if (!fits) {
    char buf[320];
    std::snprintf(buf, sizeof buf, "mixing diagnostics of max_lag %u need %.3g GB of device memory (%u B x %llu sites); "
                  "%.3g GB are free: use a smaller max_lag or more GPUs (the diagnostics are off)",
                  K, need / 1e9, per_site, (unsigned long long)at.cnt, free_b / 1e9);
    return fail(c, EPV_ERR_ARG, buf);
  }
  if (at.cnt) {
    HIP_TRY(c, hipMalloc(&c->mx.d_fp, (size_t)8u * at.cnt));
    HIP_TRY(c, hipMalloc(&c->mx.d_moved, (size_t)4u * at.cnt));
    HIP_TRY(c, hipMalloc(&c->mx.d_sums, (size_t)8u * (2u + K) * at.cnt));
    HIP_TRY(c, hipMalloc(&c->mx.d_ring, (size_t)4u * K * at.cnt));
  }
  c->mx.at = at;
  c->mx.C = c->S.C;
  return mixing_zero(c);
}
// `more` further samples fit: a site's x is at most B C, so S2 and C_k stay below 2^64 while
//   samples <= (2^64 - 1) / (B C)^2, and moved (32 bits) while samples <= 2^21.  With the capacity of now
int mixing_check_cap(epv_ctx *c, uint64_t more) {
  const uint64_t xmax = (uint64_t)c->S.B * c->S.C;   // (< 2^23: B < 2^12, C <= EPV_MAX_CAP)
  const uint64_t cap = xmax ? std::min<uint64_t>(EPV_MIX_MAX_SAMPLES, ~0ull / (xmax * xmax)) : EPV_MIX_MAX_SAMPLES;
  if (c->mx.samples <= cap && more <= cap - c->mx.samples) return EPV_OK;
  char buf[320];
  std::snprintf(buf, sizeof buf, "mixing diagnostics %s %llu samples, the most their sums take at %u branches of "
                "capacity %u: read them out and epv_reset_mixing", more == 1u ? "hold" : "would pass",
                (unsigned long long)cap, c->S.B, c->S.C);
  return fail(c, EPV_ERR_STATE, buf);
}
// the buffers match the current site range, and the samples held fit the cap of the capacity of now
int ensure_mixing(epv_ctx *c) {
  if (!(pavg_layout(c, true, true) == c->mx.at)) {
    if (c->mx.samples) return sites_changed(c, kMixing, "epv_set_mixing");
    return relayout(c, kMixing, mixing_alloc);
  }
  if (c->S.C == c->mx.C) return EPV_OK;
  c->mx.C = c->S.C;
  return mixing_check_cap(c, 0u);
}
int mixing_launch_mode(epv_ctx *c, uint32_t mode, uint32_t slot, uint32_t lags) {
  if (c->mx.at.cnt)
    hipLaunchKernelGGL(epv_mixing_accum_kernel, dim3((unsigned)((c->mx.at.cnt + 255u) / 256u)), dim3(256), 0, c->stream,
                       c->S, c->mx.at.lo, c->mx.at.cnt, c->mx.K, mode, slot, lags, c->mx.d_fp, c->mx.d_moved,
                       c->mx.d_sums, c->mx.d_ring);
  HIP_TRY(c, hipGetLastError());
  return EPV_OK;
}
// the state after burn-in opens a run: its fingerprint is kept, it is no sample (ensure_mixing first)
int begin_mixing(epv_ctx *c) {
  const int rc = mixing_launch_mode(c, EPV_MIX_OPEN, 0u, 0u);
  if (rc) return rc;
  c->mx.run_open = true;
  c->mx.run_len = 0;
  c->mx.run_sweep = c->n_sweeps;
  return EPV_OK;
}
// the resident paths as one sample (ensure_mixing first): linked to the sample (or opening state) before it when
// the run is open and exactly one sweep has passed since, else the first of a new run
int launch_mixing(epv_ctx *c) {
  int rc = mixing_check_cap(c, 1u);
  if (rc) return rc;
  MixingState &m = c->mx;
  const bool linked = m.run_open && c->n_sweeps == m.run_sweep + 1u;
  if (!linked) m.run_len = 0;
  const uint32_t lags = (uint32_t)std::min<uint64_t>(m.run_len, m.K);
  if ((rc = mixing_launch_mode(c, linked ? EPV_MIX_LINKED : EPV_MIX_FIRST, (uint32_t)(m.run_len % m.K), lags))) return rc;
  ++m.samples;
  if (linked) ++m.moved_pairs;
  for (uint32_t k = 1; k <= lags; ++k) ++m.pairs[k];
  m.run_open = true;
  ++m.run_len;
  m.run_sweep = c->n_sweeps;
  return EPV_OK;
}
const Layer kMixing = {mixing_on, ensure_mixing, mixing_check_cap, launch_mixing, mixing_off, begin_mixing,
                       "mixing diagnostics are off: epv_set_mixing first", "the mixing diagnostics"};

// ---- domain maps (epv_dmaps.h): N node rows of the state to indicate; of the tree the number of nodes and the
// root's first child matter
PartDesc dmaps_part(const epv_ctx *c, uint64_t cnt) {
  PartDesc d;
  const uint32_t N = c->S.N, K = c->dp.Z.K, LK = c->dp.Z.L[K - 1u], E = dmaps_edge_bits(LK), EW = (E + 63u) / 64u;
  d.shape = dmaps_shape(N, K, LK, cnt, c->dp.max);
  d.tree = {N, corr_child0(c)};
  d.terms = text("4 B x %u nodes x %u sizes x %llu sites of counts, 16 B x %u nodes x %u words x %llu samples of edge "
                 "records, 8 B x %u nodes x %llu words of node states", N, K, (unsigned long long)cnt, N, EW,
                 (unsigned long long)c->dp.max, N, (unsigned long long)d.shape.words);
  if (cnt < E)   // (a run's membership is decided inside two adjacent parts, never three)
    d.refusal = text("domain maps: this context counts %llu sites, fewer than the %u of an edge record (twice the largest "
                     "size %u less one): a context's stretch holds at least those (the maps are off)",
                     (unsigned long long)cnt, E, LK);
  return d;
}
const PartKind kDmapsPart = {kDmaps, "domain maps", "epv_set_domain_maps", "epv_reset_domain_maps",
                             "ask for fewer sizes or samples, or use more GPUs (the maps are off)", false, dmaps_part};
bool dmaps_on(const epv_ctx *c) { return c->dp.Z.K != 0u; }
void dmaps_off(epv_ctx *c) { part_off(c->dp); }
int dmaps_alloc(epv_ctx *c) {
  const int rc = part_alloc(c, kDmapsPart, c->dp);
  if (!rc) c->dp.child0 = corr_child0(c);
  return rc;
}
int ensure_dmaps(epv_ctx *c) { return part_ensure(c, kDmapsPart, c->dp, dmaps_alloc); }
// the edge records, and the 32-bit counts: a site adds at most one per sample
int dmaps_check_cap(epv_ctx *c, uint64_t more) {
  const int rc = part_check_cap(c, kDmapsPart, c->dp, more);
  return rc ? rc : check_cap32(c, c->dp.samples, more, "domain maps", "epv_reset_domain_maps");
}
// pack the rows, then add every site's memberships (the edge records are never read while a record has no words)
int launch_dmaps(epv_ctx *c) {
  DmapsState &p = c->dp;
  return part_sample<EPV_ROWS_NODE>(c, kDmapsPart, p, p.at.cnt != 0u, p.child0, p.state, p.shape.rows, 65535u,
    [&](uint32_t v0, uint32_t nv, const unsigned long long *bits, uint64_t words, unsigned long long *edge) {
      hipLaunchKernelGGL(epv_dmaps_member_kernel, dim3(part_chunks(words, EPV_DMAPS_CHUNK_WORDS), nv), dim3(256), 0, c->stream,
                         bits, words, p.at.cnt, v0, p.Z, (uint32_t *)p.d_acc[0], edge);
    });
}
const Layer kDmaps = {dmaps_on, ensure_dmaps, dmaps_check_cap, launch_dmaps, dmaps_off, nullptr,
                      "domain maps are off: epv_set_domain_maps first", "the domain maps"};

// ---- change tracts (epv_tracts.h): the turnover's 2 B end rows, one row of tracts per branch
PartDesc tracts_part(const epv_ctx *c, uint64_t cnt) {
  PartDesc d;
  d.shape = tracts_shape(c->S.B, cnt, c->tr.max);
  d.terms = text("16 B x %u branches x %llu samples of edge records, 16 B x %u branches x %llu words of row states", c->S.B,
                 (unsigned long long)c->tr.max, c->S.B, (unsigned long long)d.shape.words);
  return d;
}
const PartKind kTractsPart = {kTracts, "change tracts", "epv_set_change_tracts", "epv_reset_change_tracts",
                              "ask for fewer samples (the change tracts are off)", true, tracts_part};
bool tracts_on(const epv_ctx *c) { return c->tr.on; }
void tracts_off(epv_ctx *c) { part_off(c->tr); }
int tracts_alloc(epv_ctx *c) { return part_alloc(c, kTractsPart, c->tr); }
int ensure_tracts(epv_ctx *c) { return part_ensure(c, kTractsPart, c->tr, tracts_alloc); }
int tracts_check_cap(epv_ctx *c, uint64_t more) { return part_check_cap(c, kTractsPart, c->tr, more); }
// pack the turnover's rows, then count the tracts, a row of them per branch
int launch_tracts(epv_ctx *c) {
  TractsState &p = c->tr;
  const uint32_t B = p.shape.rows / 2u;
  return part_sample<EPV_ROWS_ENDS>(c, kTractsPart, p, p.at.cnt && B, 0u, 1u, B, 65534u,
    [&](uint32_t b0, uint32_t nb, const unsigned long long *bits, uint64_t words, unsigned long long *edge) {
      hipLaunchKernelGGL(epv_tract_runs_kernel, dim3(part_chunks(words, EPV_DOM_CHUNK_WORDS), nb), dim3(256), 0, c->stream, bits,
                         words, p.at.cnt, b0, (unsigned long long *)p.d_acc[0], (unsigned long long *)p.d_acc[1], edge);
    });
}
const Layer kTracts = {tracts_on, ensure_tracts, tracts_check_cap, launch_tracts, tracts_off, nullptr,
                       "change tracts are off: epv_set_change_tracts first", "the change tracts"};

// the layers in the order of the chain: run_mcmc ensures, caps and launches them in this order, so the first
// that fails is the one reported, and their kernels enter the stream in this order after every batch sweep
const Layer *const kLayers[] = {&kPavg, &kBevents, &kWstat, &kEpochs, &kOrigins, &kDomains, &kPatterns, &kTurnover, &kCorr,
                                &kMixing, &kDmaps, &kTracts};

// the global-memory slab of a proposal kernel, allocated when a launch first takes that kernel (a
// context on a large tree plans three kernels but runs one: 5 - 50 GB each at full size)
int ensure_slab(epv_ctx *c, double **slab, uint64_t *cap, uint64_t need) {
  if (need <= *cap) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  dfree(*slab);
  *cap = 0;
  HIP_TRY(c, hipMalloc(slab, need * sizeof(double)));
  *cap = need;
  return EPV_OK;
}

// ---- the launch of a colour phase: phase_plan (epv_plan.h) decides, launch_phase and its stages launch.
// Every template instantiation of a proposal kernel is named once, in the four tables below: the launches and the
// dynamic-LDS limits that epv_create raises (proposal_kernel_lds) both go through them.
using p2_kernel_t = void (*)(EpvDev, uint32_t, uint32_t, uint32_t, uint32_t, uint64_t, uint64_t, uint64_t, uint64_t,
                             uint32_t, uint32_t, uint32_t, unsigned long long *, double *, const double *, EpvFused);
// the fused phase's kernel for a tree of nn nodes: the small-tree body for 2 <= nn <= EPV_P2_SMALL_MAX,
// else (and for nn = 0) the generic one; direct: the bodies whose jump stage is run_direct (EPV_OPT_DIRECT_FUSED)
template <bool DIRECT>
p2_kernel_t fused_body(uint32_t nn) {
  switch (nn) {
    case 2: return epv_mh_propose2_kernel<true, true, 2, DIRECT>;
    case 3: return epv_mh_propose2_kernel<true, true, 3, DIRECT>;
    case 4: return epv_mh_propose2_kernel<true, true, 4, DIRECT>;
    case 5: return epv_mh_propose2_kernel<true, true, 5, DIRECT>;
    default: return epv_mh_propose2_kernel<true, true, 0, DIRECT>;
  }
}
p2_kernel_t fused_kernel(uint32_t nn, bool direct) { return direct ? fused_body<true>(nn) : fused_body<false>(nn); }
// the second proposal kernel (seg: it lists the dirty segments for the segment-parallel jump kernels), and the third
p2_kernel_t p2_kernel(bool seg) { return seg ? epv_mh_propose2_kernel<true, false> : epv_mh_propose2_kernel<false, false>; }
auto p3_kernel(uint32_t words) { return words == 2u ? epv_mh_propose3_kernel<2> : epv_mh_propose3_kernel<1>; }
// their leaf variants (EPV_OPT_LEAF_FAST with a held cell): the same arguments, then the evidence table and the mask
using leaf_arg_t = const uint32_t *;
using p2_leaf_kernel_t = void (*)(EpvDev, uint32_t, uint32_t, uint32_t, uint32_t, uint64_t, uint64_t, uint64_t, uint64_t,
                                  uint32_t, uint32_t, uint32_t, unsigned long long *, double *, const double *, EpvFused,
                                  leaf_arg_t, leaf_arg_t);
p2_leaf_kernel_t fused_leaf_kernel(uint32_t nn) {
  switch (nn) {
    case 2: return epv_mh_propose2_kernel<true, true, 2, false, leaf_arg_t, leaf_arg_t>;
    case 3: return epv_mh_propose2_kernel<true, true, 3, false, leaf_arg_t, leaf_arg_t>;
    case 4: return epv_mh_propose2_kernel<true, true, 4, false, leaf_arg_t, leaf_arg_t>;
    case 5: return epv_mh_propose2_kernel<true, true, 5, false, leaf_arg_t, leaf_arg_t>;
    default: return epv_mh_propose2_kernel<true, true, 0, false, leaf_arg_t, leaf_arg_t>;
  }
}
p2_leaf_kernel_t p2_leaf_kernel(bool seg) { return seg ? epv_mh_propose2_kernel<true, false, 0, false, leaf_arg_t, leaf_arg_t> : epv_mh_propose2_kernel<false, false, 0, false, leaf_arg_t, leaf_arg_t>; }
auto p3_leaf_kernel(uint32_t words) { return words == 2u ? epv_mh_propose3_kernel<2, leaf_arg_t, leaf_arg_t> : epv_mh_propose3_kernel<1, leaf_arg_t, leaf_arg_t>; }
// the first, by its trailing arguments: none (EPV_LEAF_DATA), the mask (_MASK), the evidence table and the mask (_EVIDENCE)
template <class... Leaf>
auto v1_kernel(bool gpool, bool refq) {
  constexpr int LEAF = (int)sizeof...(Leaf);
  return gpool ? (refq ? epv_mh_propose_kernel<true, true, LEAF, Leaf...> : epv_mh_propose_kernel<true, false, LEAF, Leaf...>)
               : (refq ? epv_mh_propose_kernel<false, true, LEAF, Leaf...> : epv_mh_propose_kernel<false, false, LEAF, Leaf...>);
}
// the proposal kernels ask for more dynamic LDS than the 64 KiB default (epv_create)
void proposal_kernel_lds() {
  auto raise = [](int kib, auto... kernels) {
    ((void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernels), hipFuncAttributeMaxDynamicSharedMemorySize, kib * 1024), ...);
  };
  raise(128, p3_kernel(1u), p3_kernel(2u), p3_leaf_kernel(1u), p3_leaf_kernel(2u));   // (it has static LDS too)
  raise(160, p2_kernel(false), p2_kernel(true), p2_leaf_kernel(false), p2_leaf_kernel(true));
  for (uint32_t nn = 0; nn <= EPV_P2_SMALL_MAX; ++nn) raise(160, fused_kernel(nn, false), fused_kernel(nn, true), fused_leaf_kernel(nn));
  for (int v = 0; v < 4; ++v)
    raise(160, v1_kernel<>(v & 1, v & 2), v1_kernel<leaf_arg_t>(v & 1, v & 2), v1_kernel<leaf_arg_t, leaf_arg_t>(v & 1, v & 2));
}

// what the stages of one colour phase share
struct PhaseArgs {
  uint32_t colour, seed_lo, seed_hi, sweep;
  uint64_t first, last, own_lo, own_hi;   // local sites the phase may update; those statistics and the accept counter cover
  uint64_t s0;                            // first local site of this colour (the kernels derive the same value)
  uint64_t threads, blocks;               // sites of this colour: a lane each; blocks of the first proposal kernel
};

// the whole phase in one kernel, one wave per fused_lanes sites (see epv_propose2.h)
int launch_fused(epv_ctx *c, const PhasePlan &P, const PhaseArgs &a) {
  const PlanV2 &v = c->shapes.v2;
  const int frc = ensure_fused_buffers(c);
  if (frc) return frc;
  const unsigned pb = (unsigned)((a.threads + v.fused_lanes - 1u) / v.fused_lanes);
  if (pb > c->fused_waves) return fail(c, EPV_ERR_STATE, "fused phase: launch larger than its lists");
  // (a lane whose worst case is beyond the pool would never run, and the kernel's round loop never end)
  if (v.pool < p2_worst_dbl(c->S.B, c->S.C, p2_hrec(true, true)))
    return fail(c, EPV_ERR_STATE, "fused phase: the record pool is below one lane's worst case");
  EpvFused F = c->F;
  F.meta_cache = P.meta_cache ? 1u : 0u;
  F.lanes = v.fused_lanes;
  F.grouped_rounds = 4u;     // rounds of the grouped search of a short segment list
  F.topo = 0u;               // small-tree body: bit node = a leaf, bits 8 + 3 node .. = the parent
  for (uint32_t node = 1; node < P.small_nn; ++node)
    F.topo |= (c->subtree[node] == 1u ? 1u << node : 0u) | (c->parent[node] << (8u + 3u * node));
  F.giveups = c->d_counters + EPV_CNT_WORDS;
  if (P.unobs || P.evidence)    // (EPV_OPT_LEAF_FAST: the plan never pairs a held cell with the direct bodies)
    hipLaunchKernelGGL(fused_leaf_kernel(P.small_nn), dim3(pb), dim3(64), v.lds, c->stream, c->S, a.colour, a.seed_lo,
                       a.seed_hi, a.sweep, a.first, a.last, a.own_lo, a.own_hi, v.pool, 0u, 0u, c->d_counters, (double *)nullptr,
                       c->d_segtab, F, (leaf_arg_t)c->d_evidence, (leaf_arg_t)c->d_unobs);
  else
  hipLaunchKernelGGL(fused_kernel(P.small_nn, P.direct), dim3(pb), dim3(64), v.lds, c->stream, c->S, a.colour, a.seed_lo,
                     a.seed_hi, a.sweep, a.first, a.last, a.own_lo, a.own_hi, v.pool, 0u, 0u, c->d_counters, (double *)nullptr,
                     c->d_segtab, F);
  return EPV_OK;
}

template <class... Leaf>
void launch_v1(epv_ctx *c, const PhasePlan &P, const PhaseArgs &a, Leaf... leaf) {
  const PlanV1 &v = c->shapes.v1;
  hipLaunchKernelGGL(v1_kernel<Leaf...>(P.gpool, P.refq), dim3((unsigned)a.blocks), dim3(v.threads), v.lds, c->stream, c->S,
                     a.colour, a.seed_lo, a.seed_hi, a.sweep, a.first, a.last, v.pool_entries, c->d_counters,
                     P.gpool ? c->d_gpool : (double *)nullptr, leaf...);
}
// the proposal stage.  list_mode: 0, or 1 + the phase parity that V2 and V3 file their listed sites under
int launch_propose(epv_ctx *c, const PhasePlan &P, const PhaseArgs &a, uint32_t list_mode) {
  if (P.propose == EPV_PLAN_V3) {
    // large tree: a 16-bit word per (node, lane) in LDS, q rows and heavy records in a slab (epv_propose3.h)
    const PlanV3 &v = c->shapes.v3;
    const int rc = ensure_slab(c, &c->d_gpool3, &c->gpool3_cap, v.slab_need);
    if (rc) return rc;
    if (P.unobs || P.evidence)
      hipLaunchKernelGGL(p3_leaf_kernel(P.p3_words), dim3((unsigned)((a.threads + 255u) / 256u)), dim3(256), v.lds, c->stream,
                         c->S, a.colour, a.seed_lo, a.seed_hi, a.sweep, a.first, a.last, a.own_lo, a.own_hi, v.list_cap, v.qrows,
                         v.n_up, v.depth, list_mode - 1u, c->d_counters, c->d_gpool3, c->d_segtab, c->d_nodetab, c->d_slabflags,
                         v.slots, (leaf_arg_t)c->d_evidence, (leaf_arg_t)c->d_unobs);
    else
    hipLaunchKernelGGL(p3_kernel(P.p3_words), dim3((unsigned)((a.threads + 255u) / 256u)), dim3(256), v.lds, c->stream, c->S,
                       a.colour, a.seed_lo, a.seed_hi, a.sweep, a.first, a.last, a.own_lo, a.own_hi, v.list_cap, v.qrows,
                       v.n_up, v.depth, list_mode - 1u, c->d_counters, c->d_gpool3, c->d_segtab, c->d_nodetab, c->d_slabflags,
                       v.slots);
    ++c->phase_parity;
  } else if (P.propose == EPV_PLAN_V2) {
    const PlanV2 &v = c->shapes.v2;
    const bool seg = P.jumps == EPV_PLAN_JUMPS_SEGMENTS;
    // (as in launch_fused: the pool may have been planned next to a fused body, whose records are shorter)
    if (v.pool < p2_worst_dbl(c->S.B, c->S.C, p2_hrec(false, seg)))
      return fail(c, EPV_ERR_STATE, "second proposal kernel: the record pool is below one lane's worst case");
    if (seg) { const int rc = ensure_seg_buffers(c); if (rc) return rc; }
    if (P.unobs || P.evidence)
      hipLaunchKernelGGL(p2_leaf_kernel(seg), dim3((unsigned)((a.threads + 63u) / 64u)), dim3(64), v.lds, c->stream, c->S,
                         a.colour, a.seed_lo, a.seed_hi, a.sweep, a.first, a.last, a.own_lo, a.own_hi, v.pool, 0u, list_mode - 1u,
                         c->d_counters, (double *)nullptr, c->d_segtab, EpvFused{}, (leaf_arg_t)c->d_evidence,
                         (leaf_arg_t)c->d_unobs);
    else
    hipLaunchKernelGGL(p2_kernel(seg), dim3((unsigned)((a.threads + 63u) / 64u)), dim3(64), v.lds, c->stream, c->S, a.colour,
                       a.seed_lo, a.seed_hi, a.sweep, a.first, a.last, a.own_lo, a.own_hi, v.pool, 0u, list_mode - 1u,
                       c->d_counters, (double *)nullptr, c->d_segtab, EpvFused{});
    ++c->phase_parity;
  } else {
    if (P.gpool) { const int rc = ensure_slab(c, &c->d_gpool, &c->gpool_cap, c->shapes.v1.slab_need); if (rc) return rc; }
    // (under evidence the mask rides along where one is held: a cell without evidence follows it)
    if (P.evidence) launch_v1(c, P, a, (leaf_arg_t)c->d_evidence, (leaf_arg_t)c->d_unobs);
    else if (P.unobs) launch_v1(c, P, a, (leaf_arg_t)c->d_unobs);
    else launch_v1(c, P, a);
  }
  return EPV_OK;
}

// the jump stage: the jump times of every dirty (site, branch) pair of the proposals
void launch_jumps(epv_ctx *c, const PhasePlan &P, const PhaseArgs &a) {
  const size_t lds = const_lds_bytes(c->S.N);
  unsigned long long *giveups = c->d_counters + EPV_CNT_WORDS;   // (the direct sampler's)
  // the sequential kernel -- under EPV_OPT_DIRECT_SAMPLER its direct variant -- on gx blocks per shard
  auto general = [&](uint64_t gx, uint32_t tpw) {
    if (P.direct)
      hipLaunchKernelGGL(epv_mh_jumps_direct_kernel, dim3((unsigned)gx, EPV_SHARDS), dim3(256), lds, c->stream, c->S, a.seed_lo,
                         a.seed_hi, a.sweep, tpw, a.s0, c->d_counters, giveups);
    else
      hipLaunchKernelGGL(epv_mh_jumps_kernel, dim3((unsigned)gx, EPV_SHARDS), dim3(256), lds, c->stream, c->S, a.seed_lo,
                         a.seed_hi, a.sweep, tpw, a.s0, 0.0, 0.0, c->d_counters, 0u);
  };
  if (P.jumps == EPV_PLAN_JUMPS_SEGMENTS) {
    // dirty segments one lane each, then their branches one lane each; both lists are sized on
    // the device, the grids cover a quarter / an eighth of the capacity and stride over the rest
    const dim3 sg((unsigned)std::min<uint64_t>(32u, std::max<uint64_t>(1u, (c->S.seg_cap / 4u + 255u) / 256u)), EPV_SHARDS);
    const dim3 bg((unsigned)std::min<uint64_t>(16u, std::max<uint64_t>(1u, (c->S.btask_cap / 8u + 255u) / 256u)), EPV_SHARDS);
    if (P.direct)
      hipLaunchKernelGGL(epv_seg_search_direct_kernel, sg, dim3(256), lds, c->stream, c->S, a.seed_lo, a.seed_hi, a.sweep,
                         c->d_counters, giveups);
    else
      hipLaunchKernelGGL(epv_seg_search_kernel, sg, dim3(256), lds, c->stream, c->S, a.seed_lo, a.seed_hi, a.sweep,
                         c->d_counters);
    hipLaunchKernelGGL(P.direct ? epv_seg_assemble_direct_kernel : epv_seg_assemble_kernel, bg, dim3(256), lds, c->stream, c->S,
                       a.seed_lo, a.seed_hi, a.sweep, a.s0, c->d_counters);
    // the sequential kernel behind them with a minimal grid: branches of more than 64 segments
    // and whatever did not fit the lists (normally nothing: it reads empty lists and leaves)
    return general(1u, 32u);
  }
  // one lane per dirty (site, branch) pair; the count is only known on the device, so
  // launch a grid that covers the typical case and grid-stride over the rest
  const uint64_t max_tasks = a.blocks / EPV_SHARDS * 64u * c->S.B + 64u * c->S.B;  // per shard
  // lanes of a wave that own a task (the others only help in the cooperative search): full
  // waves when there is work for every SIMD, fewer tasks per wave -- a shorter critical path --
  // on a small genome (measured: DESIGN.md section 4.1)
  const double est = (double)a.threads * c->S.B * std::min(1.0, 0.1 + c->kbar) / 2048.0;
  const uint32_t tpw = est >= 64.0 ? 64u : est >= 32.0 ? 32u : est >= 16.0 ? 16u : 8u;
  // the one-segment tasks in their own lean kernel (phase_plan), the general one then takes the rest
  // with a grid sized for it; a block (4 waves) takes 4*tpw tasks per pass; size the grid for ~1/4 of the worst case
  if (P.jumps != EPV_PLAN_JUMPS_ALL) return general(std::min<uint64_t>((max_tasks / 4u + 4u * tpw - 1u) / (4u * tpw) + 1u, 256u), tpw);
  const uint64_t j1b = std::min<uint64_t>((max_tasks / 4u + 255u) / 256u + 1u, 256u);
  const uint64_t jgb = std::min<uint64_t>((max_tasks / 16u + 4u * tpw - 1u) / (4u * tpw) + 1u, 64u);
  hipLaunchKernelGGL(epv_mh_jumps_all_kernel, dim3(EPV_SHARDS, (unsigned)(jgb + j1b)), dim3(256), lds, c->stream, c->S,
                     a.seed_lo, a.seed_hi, a.sweep, tpw, a.s0, c->d_counters, (uint32_t)jgb);
}

// the accept stage, over the listed sites (list_mode != 0) or over every site of the colour
void launch_accept(epv_ctx *c, const PhasePlan &P, const PhaseArgs &a, uint32_t list_mode) {
  // the listed sites (proposal differs from the current path) per shard: typically ~30 % of the colour
  const uint64_t per_shard = (a.threads + EPV_SHARDS - 1u) / EPV_SHARDS;
  if (P.accept == EPV_PLAN_ACCEPT_V3) {
    // large trees (no room for the meta cache): a lane per (site, triple), branches in groups (epv_accept3.h);
    // unlisted, every site of the colour in one row of blocks (reference proposal arithmetic on a large tree)
    const uint64_t sites = list_mode ? per_shard : a.threads;
    const unsigned ax3 = (unsigned)std::max<uint64_t>(1u, (sites + 4u * EPV_ACC3_SITES - 1u) / (4u * EPV_ACC3_SITES));
    hipLaunchKernelGGL(epv_mh_accept3_kernel, dim3(ax3, list_mode ? EPV_SHARDS : 1u), dim3(256), const_lds_bytes(c->S.N),
                       c->stream, c->S, a.colour, a.seed_lo, a.seed_hi, a.sweep, a.first, a.last, a.own_lo, a.own_hi,
                       c->d_counters, list_mode, list_mode ? (uint64_t)0 : a.threads);
    return;
  }
  // meta cache of the accept kernel: 5 columns x B words per lane in LDS while that stays small
  // (B <= 8: 20 KB per block next to the 24 KB of accumulators)
  const uint32_t meta_cache = P.meta_cache ? 1u : 0u;
  const size_t acc_lds = const_lds_bytes(c->S.N) + (meta_cache ? (size_t)5u * c->S.B * 256u * sizeof(epv_meta_t) : 0u);
  // listed: the grid covers half of the worst case and strides over the rest
  // (on a large tree nearly every site is listed -- one clean proposal in thirty branches is rare --
  // and a block that strides twice runs two of the kernel's long dependent chains back to back)
  const uint64_t covered = c->S.B > 8u ? per_shard : per_shard / 2u;
  const dim3 grid = list_mode ? dim3((unsigned)std::max<uint64_t>(1u, (covered + 255u) / 256u), EPV_SHARDS)
                              : dim3((unsigned)((a.threads + 255u) / 256u));
  hipLaunchKernelGGL(epv_mh_accept_kernel, grid, dim3(256), acc_lds, c->stream, c->S, a.colour, a.seed_lo, a.seed_hi, a.sweep,
                     a.first, a.last, a.own_lo, a.own_hi, c->d_counters, list_mode, meta_cache);
}

int launch_phase(epv_ctx *c, int colour, uint64_t seed, uint32_t sweep) {
  PhaseArgs a{(uint32_t)colour, (uint32_t)seed, (uint32_t)(seed >> 32), sweep};
  int prc = phase_range(c, &a.first, &a.last);
  if (prc) return prc;
  owned_range(c, &a.own_lo, &a.own_hi);
  const uint64_t span = a.last - a.first + 1u;
  a.threads = (span + 2u) / 3u;
  a.s0 = a.first + ((a.colour + 3u - (uint32_t)((c->S.g0 + a.first) % 3u)) % 3u);
  a.blocks = (a.threads + c->shapes.v1.threads - 1u) / c->shapes.v1.threads;
  if (a.blocks == 0) return EPV_OK;
  // the guard of the fixed sites of this colour (epv_regions.h): kept before the phase, put back after it
  const uint64_t *fx_sites = c->fx.d_sites + c->fx.off[colour];
  const uint64_t fx_count = c->fx.off[colour + 1] - c->fx.off[colour];
  hipEvent_t e0 = nullptr, e1 = nullptr;
  c->timing = c->timing_every && (c->timing_seen++ % c->timing_every) == 0u;
  if (c->timing) {
    if (c->ev_used == c->ev_pool.size()) {
      HIP_TRY(c, hipEventCreate(&e0));
      HIP_TRY(c, hipEventCreate(&e1));
      c->ev_pool.emplace_back(e0, e1);
    }
    e0 = c->ev_pool[c->ev_used].first;
    e1 = c->ev_pool[c->ev_used].second;
    ++c->ev_used;
    HIP_TRY(c, hipEventRecord(e0, c->stream));
  }
  const PhasePlan P = phase_plan(c);
  // (the second and third proposal kernel and the fused phase count a proposal equal to the current path themselves)
  const uint32_t fx_ident = P.propose == EPV_PLAN_FUSED || P.propose == EPV_PLAN_V2 || P.propose == EPV_PLAN_V3 ? 1u : 0u;
  if (fx_count)
    hipLaunchKernelGGL(epv_fixed_save_kernel, dim3((unsigned)((fx_count + 63u) / 64u)), dim3(64), 0, c->stream, c->S,
                       fx_sites, fx_count, c->fx.save, fx_ident);
  const uint32_t list_mode = P.listed ? 1u + (c->phase_parity & 1u) : 0u;   // (never with the fused phase)
  const int rc = P.propose == EPV_PLAN_FUSED ? launch_fused(c, P, a) : launch_propose(c, P, a, list_mode);
  if (rc) return rc;
  if (P.propose != EPV_PLAN_FUSED) {
    launch_jumps(c, P, a);
    launch_accept(c, P, a, list_mode);
  }
  if (c->timing) HIP_TRY(c, hipEventRecord(e1, c->stream));
  if (fx_count)
    hipLaunchKernelGGL(epv_fixed_restore_kernel, dim3((unsigned)((fx_count + 63u) / 64u)), dim3(64), 0, c->stream, c->S,
                       fx_sites, fx_count, c->fx.save, a.first, a.last, a.own_lo, a.own_hi, fx_ident, c->d_counters);
  HIP_TRY(c, hipGetLastError());
  if (c->halo_mode) ++c->phases_used;
  return EPV_OK;
}

// fold finished timing events into the running totals (stream must be idle)
int drain_timing(epv_ctx *c) {
  for (size_t i = 0; i < c->ev_used; ++i) {
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev_pool[i].first, c->ev_pool[i].second));
    c->timed_ms += ms;
    ++c->timed_launches;
  }
  c->ev_used = 0;
  return EPV_OK;
}

int read_counters(epv_ctx *c, unsigned long long out[EPV_CNT_N]) {
  unsigned long long *raw = c->h_counters;
  HIP_TRY(c, hipMemcpyAsync(raw, c->d_counters, sizeof(unsigned long long) * EPV_CNT_WORDS,
                            hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (uint32_t k = 0; k < EPV_CNT_N; ++k) {
    out[k] = 0;
    for (uint32_t s = 0; s < EPV_SHARDS; ++s) out[k] += raw[EPV_CNT_IDX(k, s)];
  }
  return drain_timing(c);
}

int check_ready(epv_ctx *c, bool need_reset) {
  if (!c) return EPV_ERR_ARG;
  if (!c->have_tree || !c->have_model || !c->have_paths)
    return fail(c, EPV_ERR_STATE, "tree, model and paths must be set first");
  if (need_reset && !c->have_reset) return fail(c, EPV_ERR_STATE, "epv_reset has not been called");
  return EPV_OK;
}

// ---- what the entry points of every summary layer begin with
// an entry point that needs the layer on: a context, the layer on (or its message), the context's device current
int layer_entry(epv_ctx *c, const Layer &L) {
  if (!c) return EPV_ERR_ARG;
  if (!L.on(c)) return fail(c, EPV_ERR_STATE, L.off_msg);
  HIP_TRY(c, hipSetDevice(c->device));
  return EPV_OK;
}
// a setter told to switch its layer off
int layer_set_off(epv_ctx *c, const Layer &L) {
  if (!c) return EPV_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  L.off(c);
  return EPV_OK;
}
// ---- fixed sites and the layers.  Seven layers count triples or runs across neighbouring sites and are not cut at
// fixed sites yet: they and the fixed sites refuse each other, each naming the other
struct SpanningLayer {
  const Layer *L;
  const char *setter;
};
const SpanningLayer kSpanning[] = {{&kWstat, "epv_set_window_stats"},         {&kEpochs, "epv_set_epoch_stats"},
                                   {&kDomains, "epv_set_domain_stats"},       {&kTurnover, "epv_set_domain_turnover"},
                                   {&kTracts, "epv_set_change_tracts"},       {&kCorr, "epv_set_spatial_correlation"},
                                   {&kDmaps, "epv_set_domain_maps"}};
// what a spanning layer's setter begins with when it is told to switch the layer on
int refuse_fixed(epv_ctx *c, const Layer &L) {
  if (!c || c->fx.mask.empty()) return EPV_OK;
  for (const SpanningLayer &sp : kSpanning)
    if (sp.L == &L)
      return fail(c, EPV_ERR_STATE, std::string(sp.setter) + ": fixed sites are held (epv_set_fixed_sites) and " + L.name +
                                    " would count across them: clear the fixed sites first");
  return EPV_OK;
}
// a setter that has taken its arguments into the layer's state: lay out for the context as it is now
int layer_set_on(epv_ctx *c, const Layer &L, int (*alloc)(epv_ctx *)) {
  HIP_TRY(c, hipSetDevice(c->device));
  const int rc = relayout(c, L, alloc);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}
// epv_accumulate_*: the resident paths as one sample of the layer
int layer_accumulate(epv_ctx *c, const Layer &L) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (!L.on(c)) return fail(c, EPV_ERR_STATE, L.off_msg);
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = L.ensure(c)) || (rc = L.launch(c))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}

// window sums of `rows` uint32 rows [rows][at.cnt] over the sites of pavg_range (the branch events, the change
// patterns): sums[row][w - first_window] through epv_bevents_window_kernel, this context's contribution
int row_window_sums(epv_ctx *c, const uint32_t *acc, uint64_t rows, const SiteLayout &at, unsigned long long **d_out,
                    uint64_t *out_cap, uint64_t W, uint64_t first_window, uint64_t n_windows, uint64_t *sums) {
  if (!sums) return fail(c, EPV_ERR_ARG, "null output");
  if (W == 0) return fail(c, EPV_ERR_ARG, "a window holds at least one site");
  if (first_window + n_windows < first_window) return fail(c, EPV_ERR_ARG, "window range overflows");
  if (n_windows == 0) return EPV_OK;
  const uint64_t bytes = rows * n_windows * 8u;
  if (at.cnt == 0 || at.ng == 0) {   // this context counts no site
    std::memset(sums, 0, bytes);
    return EPV_OK;
  }
  const int rc = grow_staging(c, d_out, out_cap, bytes);
  if (rc) return rc;
  if (W > at.ng) W = at.ng;   // one window holds the genome: the same sums, and w W cannot overflow
  uint32_t Wp = 256u;
  if (W <= 64u) for (Wp = 1u; Wp < W; Wp <<= 1) {}
  const uint64_t per_block = 256u / Wp, blocks = (n_windows + per_block - 1u) / per_block;
  if (blocks > 0x7fffffffull) return fail(c, EPV_ERR_ARG, "too many windows in one call: read them out in pieces");
  hipLaunchKernelGGL(epv_bevents_window_kernel, dim3((unsigned)blocks, (unsigned)rows), dim3(256), 0, c->stream, acc,
                     at.B, at.cnt, at.g0 + at.lo, at.ng, W, Wp, first_window, n_windows, *d_out);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(sums, *d_out, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}

}  // namespace

EPV_API epv_ctx *epv_create(int device_id) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device_id < 0 || device_id >= count) return nullptr;
  if (hipSetDevice(device_id) != hipSuccess) return nullptr;
  epv_ctx *c = new epv_ctx();
  c->device = device_id;
  c->knobs = read_knobs(std::getenv);
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
      hipMalloc(&c->d_model, sizeof(EpvModelConst)) != hipSuccess ||
      // (one word behind the sharded counters: the direct sampler's give-ups, epv_direct_giveups)
      hipMalloc(&c->d_counters, sizeof(unsigned long long) * (EPV_CNT_WORDS + 1u)) != hipSuccess ||
      hipHostMalloc(&c->h_counters, sizeof(unsigned long long) * EPV_CNT_WORDS) != hipSuccess ||
      hipMalloc(&c->d_cnt_snap, sizeof(unsigned long long) * EPV_CNT_WORDS) != hipSuccess ||
      hipHostMalloc(&c->h_cnt_snap, sizeof(unsigned long long) * EPV_CNT_WORDS) != hipSuccess ||
      hipMemset(c->d_counters, 0, sizeof(unsigned long long) * (EPV_CNT_WORDS + 1u)) != hipSuccess) {
    delete c;
    return nullptr;
  }
  proposal_kernel_lds();
  return c;
}

EPV_API void epv_destroy(epv_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  free_paths(c);
  dfree(c->d_model); dfree(c->d_parent); dfree(c->d_subtree); dfree(c->d_blen);
  dfree(c->d_counters); dfree(c->d_sweep_tot); dfree(c->d_statscale); dfree(c->d_scale); dfree(c->d_indep); dfree(c->d_gpool); dfree(c->d_stage); dfree(c->d_lvl); dfree(c->d_gpool3); dfree(c->d_segtab); dfree(c->d_nodetab); dfree(c->d_slabflags);
  for (const Layer *L : kLayers) L->off(c);
  if (c->h_counters) (void)hipHostFree(c->h_counters);
  if (c->h_cnt_snap) (void)hipHostFree(c->h_cnt_snap);
  if (c->h_tot) (void)hipHostFree(c->h_tot);
  if (c->h_model) (void)hipHostFree(c->h_model);
  for (hipEvent_t &e : c->ev_model) if (e) { (void)hipEventDestroy(e); e = nullptr; }
  for (hipEvent_t &e : c->ev_copy) if (e) { (void)hipEventDestroy(e); e = nullptr; }
  dfree(c->d_cnt_snap);
  for (auto &p : c->ev_pool) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
  (void)hipStreamDestroy(c->stream);
  delete c;
}

EPV_API const char *epv_last_error(const epv_ctx *c) { return c ? c->err.c_str() : "null context"; }

EPV_API int epv_set_tree(epv_ctx *c, int n_nodes, const uint32_t *parent_ids,
                         const uint32_t *subtree_sizes, const double *branches) {
  if (!c) return EPV_ERR_ARG;
  if (n_nodes < 2 || n_nodes > 4095 || !parent_ids || !subtree_sizes || !branches)
    return fail(c, EPV_ERR_ARG, "bad tree");
  if (c->have_paths && (uint32_t)n_nodes != c->S.N)
    return fail(c, EPV_ERR_ARG, "tree size differs from the uploaded paths");
  for (int i = 1; i < n_nodes; ++i)
    if (parent_ids[i] >= (uint32_t)i || subtree_sizes[i] < 1 || i + subtree_sizes[i] > (uint32_t)n_nodes ||
        !(branches[i] > 0.0))
      return fail(c, EPV_ERR_ARG, "tree arrays are not a valid pre-order tree with positive branches");
  HIP_TRY(c, hipSetDevice(c->device));
  // the mask of unobserved cells and the evidence table hold rows for the leaves of the tree they were set on
  if ((c->d_unobs || c->d_evidence) && !std::equal(c->subtree.begin(), c->subtree.end(), subtree_sizes)) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    dfree(c->d_unobs);
    c->unobs_cells = 0;
    dfree(c->d_evidence);
    c->evidence_cells = 0;
  }
  c->parent.assign(parent_ids, parent_ids + n_nodes);
  c->subtree.assign(subtree_sizes, subtree_sizes + n_nodes);
  c->blen.assign(branches, branches + n_nodes);
  dfree(c->d_parent); dfree(c->d_subtree); dfree(c->d_blen); dfree(c->d_statscale); dfree(c->d_scale);
  c->statscale.clear();
  HIP_TRY(c, hipMalloc(&c->d_parent, sizeof(uint32_t) * n_nodes));
  HIP_TRY(c, hipMalloc(&c->d_subtree, sizeof(uint32_t) * n_nodes));
  HIP_TRY(c, hipMalloc(&c->d_blen, sizeof(double) * n_nodes));
  HIP_TRY(c, hipMalloc(&c->d_statscale, sizeof(double) * n_nodes));
  HIP_TRY(c, hipMalloc(&c->d_scale, sizeof(double) * n_nodes));
  HIP_TRY(c, hipMemcpy(c->d_parent, parent_ids, sizeof(uint32_t) * n_nodes, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_subtree, subtree_sizes, sizeof(uint32_t) * n_nodes, hipMemcpyHostToDevice));
  HIP_TRY(c, hipMemcpy(c->d_blen, branches, sizeof(double) * n_nodes, hipMemcpyHostToDevice));
  c->S.N = (uint32_t)n_nodes;
  c->S.B = (uint32_t)n_nodes - 1u;
  c->S.parent = c->d_parent;
  c->S.subtree = c->d_subtree;
  c->S.blen = c->d_blen;
  c->have_tree = true;
  c->have_reset = false;
  if (c->have_paths) return plan_kernels(c);
  return EPV_OK;
}

EPV_API int epv_set_model(epv_ctx *c, const double *triplet_rates, const double *T) {
  if (!c) return EPV_ERR_ARG;
  if (!triplet_rates || !T) return fail(c, EPV_ERR_ARG, "null model");
  for (int i = 0; i < 8; ++i) {
    if (!(triplet_rates[i] > 0.0)) return fail(c, EPV_ERR_ARG, "triplet rates must be positive");
    c->model.rates[i] = triplet_rates[i];
    c->model.log_rates[i] = std::log(triplet_rates[i]);  // SingleSiteSampler.cpp:464-468
  }
  for (int i = 0; i < 4; ++i) c->model.T[i] = T[i];
  HIP_TRY(c, hipSetDevice(c->device));
  // stream-ordered: the kernels already queued read the old constants, those launched after this call the new
  // ones, and the host waits for neither.  The copy leaves from a pinned slot; the two slots take turns, and a
  // slot is written only after the copy that last read it has passed.
  if (!c->h_model) HIP_TRY(c, hipHostMalloc(&c->h_model, 2u * sizeof(EpvModelConst)));
  const uint32_t slot = c->model_slot;
  if (!c->ev_model[slot]) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_model[slot], hipEventDisableTiming));
  else HIP_TRY(c, hipEventSynchronize(c->ev_model[slot]));
  c->h_model[slot] = c->model;
  HIP_TRY(c, hipMemcpyAsync(c->d_model, &c->h_model[slot], sizeof(EpvModelConst), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev_model[slot], c->stream));
  c->model_slot = slot ^ 1u;
  c->S.model = c->d_model;
  c->have_model = true;
  c->have_reset = false;
  return EPV_OK;
}

// device storage of n_sites x B paths with `capacity` jump slots each (both buffers), the phase
// hand-over arrays and the work lists; the paths themselves are filled in by the caller
static int alloc_paths(epv_ctx *c, uint64_t n_sites, uint32_t capacity, uint64_t global_site_offset) {
  const uint64_t B = c->S.B, E = B * n_sites;
  HIP_TRY(c, hipSetDevice(c->device));
  free_paths(c);
  mixing_close_run(c);   // (other paths: no sample is linked to them)
  c->S.n = n_sites;
  c->S.g0 = global_site_offset;
  c->S.n_global = global_site_offset + n_sites;
  c->S.C = capacity;
  HIP_TRY(c, hipMalloc(&c->S.meta, 2u * E * sizeof(epv_meta_t)));
  HIP_TRY(c, hipMalloc(&c->S.jumps, 2u * E * capacity * sizeof(double)));
  HIP_TRY(c, hipMalloc(&c->S.sel, n_sites));
  HIP_TRY(c, hipMalloc(&c->S.tri, n_sites * sizeof(double)));
  c->S.phase_cap = epv_phase_cap(n_sites);
  HIP_TRY(c, hipMalloc(&c->S.prop_llr, c->S.phase_cap * sizeof(double)));
  HIP_TRY(c, hipMalloc(&c->S.prop_flag, c->S.phase_cap));
  c->S.W = (2u * capacity + 1u + 63u) / 64u;
  HIP_TRY(c, hipMalloc(&c->S.prop_states, B * c->S.phase_cap * c->S.W * sizeof(uint64_t)));
  // one task region per counter shard, sized for the worst case of the blocks that use it
  c->S.task_cap = epv_task_cap(n_sites, B);
  HIP_TRY(c, hipMalloc(&c->S.tasks, c->S.task_cap * EPV_SHARDS * 2u * sizeof(unsigned long long)));
  // segment-parallel jump sampling: branch list as large as the task regions, segment list for
  // the expected number of dirty segments with a wide margin (what does not fit falls back to the
  // sequential kernel's lists)
  //   (allocated by ensure_seg_buffers when that path is first used)
  c->S.btask_cap = c->S.seg_cap = 0;
  // accept list: one region per counter shard, room for every site of the blocks that use it
  c->S.alist_cap = epv_task_cap(n_sites, 1u);
  HIP_TRY(c, hipMalloc(&c->S.alist, c->S.alist_cap * EPV_SHARDS * sizeof(uint32_t)));
  HIP_TRY(c, hipMemsetAsync(c->S.meta, 0, 2u * E * sizeof(epv_meta_t), c->stream));
  c->first = 1;
  c->last = n_sites - 2;
  c->halo_mode = false;
  c->halo_left = c->halo_right = 0;
  c->phases_used = 0;
  return EPV_OK;
}

EPV_API int epv_upload_paths(epv_ctx *c, uint64_t n_sites, const uint8_t *init_state,
                             const uint64_t *offsets, const double *jumps, uint32_t capacity,
                             uint64_t global_site_offset) {
  if (!c) return EPV_ERR_ARG;
  if (!c->have_tree) return fail(c, EPV_ERR_STATE, "epv_set_tree must come before epv_upload_paths");
  if (n_sites < 3 || !init_state || !offsets) return fail(c, EPV_ERR_ARG, "bad paths");
  if (global_site_offset + n_sites > 0xffffffffull)
    return fail(c, EPV_ERR_ARG, "site indices must fit 32 bits (Philox counter word)");
  const uint64_t B = c->S.B, E = B * n_sites;
  uint64_t maxj = 0;
  for (uint64_t e = 0; e < E; ++e) {
    if (offsets[e + 1] < offsets[e]) return fail(c, EPV_ERR_ARG, "offsets must be non-decreasing");
    maxj = std::max<uint64_t>(maxj, offsets[e + 1] - offsets[e]);
  }
  if (capacity == 0) capacity = (uint32_t)std::max<uint64_t>(16u, 2u * maxj + 8u);
  if (capacity > EPV_MAX_CAP) capacity = EPV_MAX_CAP;
  if (maxj > capacity) return fail(c, EPV_ERR_CAPACITY, "an input path has more jumps than the capacity");
  int arc = alloc_paths(c, n_sites, capacity, global_site_offset);
  if (arc) return arc;
  c->kbar = E ? (double)offsets[E] / (double)E : 0.0;
  // staging of the CSR form
  DevTmp<uint8_t> d_init;
  DevTmp<uint64_t> d_off;
  DevTmp<double> d_j;
  const uint64_t tot = offsets[E];
  HIP_TRY(c, d_init.alloc(E));
  HIP_TRY(c, d_off.alloc(E + 1));
  HIP_TRY(c, d_j.alloc(std::max<uint64_t>(tot, 1)));
  HIP_TRY(c, hipMemcpyAsync(d_init.p, init_state, E, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d_off.p, offsets, (E + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  if (tot) HIP_TRY(c, hipMemcpyAsync(d_j.p, jumps, tot * sizeof(double), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(epv_scatter_kernel, dim3((unsigned)((E + 255u) / 256u)), dim3(256), 0, c->stream,
                     c->S, d_init.p, d_off.p, d_j.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->have_paths = true;
  c->have_reset = false;
  return plan_kernels(c);
}

// epievo_sim's forward simulation on the device (epv_forward.h): root sequence (given, or
// EpiEvoModel::sample_state_sequence with keyed uniforms), then every branch in pre-order by
// site-parallel thinning.  The histories end up resident like uploaded paths.
EPV_API int epv_forward_simulate(epv_ctx *c, uint64_t n_sites, const uint8_t *root_states, uint64_t seed,
                                 uint32_t capacity, uint64_t *total_jumps) {
  if (!c) return EPV_ERR_ARG;
  if (!c->have_tree || !c->have_model)
    return fail(c, EPV_ERR_STATE, "epv_set_tree and epv_set_model must come before epv_forward_simulate");
  if (n_sites < 3 || n_sites > 0xffffffffull) return fail(c, EPV_ERR_ARG, "bad number of sites");
  if (capacity == 0) capacity = 16u;
  if (capacity > EPV_MAX_CAP) capacity = EPV_MAX_CAP;
  const auto t_begin = std::chrono::steady_clock::now();
  int rc = alloc_paths(c, n_sites, capacity, 0);
  if (rc) return rc;
  const uint64_t n = n_sites, N = c->S.N;
  const uint32_t seed_lo = (uint32_t)seed, seed_hi = (uint32_t)(seed >> 32);
  EpvFwd F{};
  DevTmp<uint8_t> st0, st1, endv, agg, prefix;
  DevTmp<uint32_t> k0, k1;
  DevTmp<double> t0, t1;
  DevTmp<unsigned long long> info;
  HIP_TRY(c, st0.alloc(n)); HIP_TRY(c, st1.alloc(n));
  HIP_TRY(c, k0.alloc(n)); HIP_TRY(c, k1.alloc(n));
  HIP_TRY(c, t0.alloc(n)); HIP_TRY(c, t1.alloc(n));
  HIP_TRY(c, endv.alloc(N * n));
  HIP_TRY(c, info.alloc(3));
  F.st[0] = st0.p; F.st[1] = st1.p; F.k[0] = k0.p; F.k[1] = k1.p; F.t[0] = t0.p; F.t[1] = t1.p; F.end = endv.p;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const auto t_alloc = std::chrono::steady_clock::now();
  F.lam_max = c->model.rates[0];
  for (int i = 1; i < 8; ++i) F.lam_max = std::max(F.lam_max, c->model.rates[i]);
  for (int i = 0; i < 8; ++i) F.pacc[i] = c->model.rates[i] / F.lam_max;
  if (root_states) {
    HIP_TRY(c, hipMemcpyAsync(F.end, root_states, n, hipMemcpyHostToDevice, c->stream));
  } else {
    const uint64_t per_block = 256u * EPV_ROOT_PER_THREAD, nb = (n + per_block - 1u) / per_block;
    HIP_TRY(c, agg.alloc(nb)); HIP_TRY(c, prefix.alloc(nb));
    const double T00 = c->model.T[0], T11 = c->model.T[3], pi1 = (1.0 - T00) / (2.0 - T11 - T00);   // EpiEvoModel.cpp:289
    hipLaunchKernelGGL(epv_fwd_root_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, n, (uint64_t)0, seed_lo, seed_hi,
                       T00, T11, pi1, 0u, agg.p, (const uint8_t *)nullptr, (uint8_t *)nullptr);
    hipLaunchKernelGGL(epv_fwd_root_scan_kernel, dim3(1), dim3(64), 0, c->stream, agg.p, nb, prefix.p);
    hipLaunchKernelGGL(epv_fwd_root_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, n, (uint64_t)0, seed_lo, seed_hi,
                       T00, T11, pi1, 1u, agg.p, prefix.p, F.end);
  }
  HIP_TRY(c, hipGetLastError());
  // tiles of EPV_FWD_THREADS sites with `halo` redundant ones on each side, `rounds` rounds a launch
  const uint32_t halo = 16u, rounds = 64u, own_w = EPV_FWD_THREADS - 2u * halo;
  const unsigned tiles = (unsigned)((n + own_w - 1u) / own_w);
  unsigned long long h_info[3] = {0ull, 0ull, 0ull};
  uint64_t tot = 0;
  for (uint32_t node = 1; node < N; ++node) {
    uint32_t p = 0u;
    hipLaunchKernelGGL(epv_fwd_begin_kernel, dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, c->stream, c->S, F, node,
                       c->parent[node], seed_lo, seed_hi, p);
    for (uint32_t launch = 0;; ++launch) {
      HIP_TRY(c, hipMemsetAsync(info.p, 0, 3 * sizeof(unsigned long long), c->stream));
      hipLaunchKernelGGL(epv_fwd_rounds_kernel, dim3(tiles), dim3(EPV_FWD_THREADS), 0, c->stream, c->S, F, node,
                         c->blen[node], seed_lo, seed_hi, p, halo, rounds, info.p);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(h_info, info.p, sizeof h_info, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      p ^= 1u;
      tot += h_info[2];
      if (h_info[1]) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "forward simulation: %llu paths of node %u need more than %u jump slots; "
                      "call again with a larger capacity", h_info[1], node, capacity);
        free_paths(c);
        return fail(c, EPV_ERR_CAPACITY, buf);
      }
      if (h_info[0] == 0ull) break;
      if (launch > 100000u) { free_paths(c); return fail(c, EPV_ERR_STATE, "forward simulation does not terminate"); }
    }
  }
  c->have_paths = true;
  c->have_reset = false;
  if (total_jumps) *total_jumps = tot;
  c->kbar = (double)tot / (double)(c->S.B * n);
  const auto t_end = std::chrono::steady_clock::now();
  c->fwd_alloc_ms = std::chrono::duration<double, std::milli>(t_alloc - t_begin).count();
  c->fwd_sim_ms = std::chrono::duration<double, std::milli>(t_end - t_alloc).count();
  return plan_kernels(c);
}

EPV_API int epv_forward_last_ms(epv_ctx *c, double *alloc_ms, double *simulate_ms) {
  if (!c || !alloc_ms || !simulate_ms) return EPV_ERR_ARG;
  *alloc_ms = c->fwd_alloc_ms;
  *simulate_ms = c->fwd_sim_ms;
  return EPV_OK;
}

static int finish_mcmc(epv_ctx *c, uint64_t *n_accepted, uint64_t acc_base);

EPV_API int epv_set_options(epv_ctx *c, uint32_t flags) {
  if (!c) return EPV_ERR_ARG;
  if (flags & ~(uint32_t)(EPV_OPT_REFERENCE_PROPOSAL_RATIO | EPV_OPT_FORWARD_REJECTION | EPV_OPT_SAMPLE_ROOT |
                          EPV_OPT_DIRECT_SAMPLER | EPV_OPT_DIRECT_FUSED | EPV_OPT_LEAF_FAST))
    return fail(c, EPV_ERR_ARG, "unknown option bits");
  if ((flags & EPV_OPT_DIRECT_FUSED) && !(flags & EPV_OPT_DIRECT_SAMPLER))
    return fail(c, EPV_ERR_ARG, "EPV_OPT_DIRECT_FUSED selects the fused body of EPV_OPT_DIRECT_SAMPLER: set both");
  if ((flags & EPV_OPT_DIRECT_SAMPLER) && (flags & EPV_OPT_FORWARD_REJECTION))
    return fail(c, EPV_ERR_ARG, "EPV_OPT_DIRECT_SAMPLER and EPV_OPT_FORWARD_REJECTION name two samplers: set one");
  static_assert(EPV_OPT_DIRECT_SAMPLER == EPV_FLAG_DIRECT_SAMPLER && EPV_OPT_DIRECT_FUSED == EPV_FLAG_DIRECT_FUSED &&
                EPV_OPT_LEAF_FAST == EPV_FLAG_LEAF_FAST, "option bits");
  static_assert(EPV_OPT_REFERENCE_PROPOSAL_RATIO == EPV_FLAG_REFERENCE_PROPOSAL_RATIO &&
                EPV_OPT_FORWARD_REJECTION == EPV_FLAG_FORWARD_REJECTION && EPV_OPT_SAMPLE_ROOT == EPV_FLAG_SAMPLE_ROOT,
                "option bits");
  c->S.flags = flags;
  return EPV_OK;
}
EPV_API int epv_get_options(epv_ctx *c, uint32_t *flags) {
  if (!c || !flags) return EPV_ERR_ARG;
  *flags = c->S.flags;
  return EPV_OK;
}

EPV_API int epv_phase_mode(epv_ctx *c, uint32_t *mode) {
  if (!c || !mode || !c->have_paths) return EPV_ERR_ARG;
  const PhasePlan P = phase_plan(c);
  *mode = P.propose == EPV_PLAN_V3 ? EPV_PHASE_V3 : P.propose == EPV_PLAN_FUSED ? EPV_PHASE_FUSED
        : P.propose == EPV_PLAN_V1 ? EPV_PHASE_V1 : P.jumps == EPV_PLAN_JUMPS_SEGMENTS ? EPV_PHASE_V2_SEGMENTS : EPV_PHASE_V2;
  return EPV_OK;
}

EPV_API int epv_phase_plan(epv_ctx *c, uint32_t *word) {
  if (!c || !word || !c->have_paths) return EPV_ERR_ARG;
  *word = phase_plan(c).word();
  return EPV_OK;
}

// known-answer entry for the device's Philox blocks: every form a kernel may inline (epv_philox.h) at
// call sites with run-time and with compile-time-zero counter fields
__global__ void epv_philox_kat_kernel(uint32_t seed_lo, uint32_t seed_hi, uint32_t n, const uint32_t *ctr, double *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t site = ctr[6u * i], sweep = ctr[6u * i + 1u], b = ctr[6u * i + 2u], k = ctr[6u * i + 3u];
  const uint32_t t = ctr[6u * i + 4u], blk = ctr[6u * i + 5u];
  const epv_block2 a = epv_keyed_block<true>(seed_lo, seed_hi, site, sweep, b, k, t, blk);
  epv_block2 p = epv_keyed_block<false>(seed_lo, seed_hi, site, sweep, b, k, t, blk);
  epv_block2 f = p;       // the folded call sites, where the counter allows them
  if (t == 0u && blk == 0u) f = epv_keyed_block<false>(seed_lo, seed_hi, site, sweep, b, k, 0u, 0u);
  if (t == 0u && blk == 0u && k == 0u) p = epv_keyed_block<false>(seed_lo, seed_hi, site, sweep, b, 0u, 0u, 0u);
  if (t == 0u && blk == 0u && k == 0u && b == 0u) f = epv_keyed_block<false>(seed_lo, seed_hi, site, sweep, 0u, 0u, 0u, 0u);
  out[6u * i] = a.d0; out[6u * i + 1u] = a.d1;
  out[6u * i + 2u] = p.d0; out[6u * i + 3u] = p.d1;
  out[6u * i + 4u] = f.d0; out[6u * i + 5u] = f.d1;
}

EPV_API int epv_philox_kat(epv_ctx *c, uint64_t seed, uint32_t n, const uint32_t *counters, double *out) {
  if (!c || !counters || !out || !n || n > (1u << 20)) return EPV_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  uint32_t *d_ctr = nullptr;
  double *d_out = nullptr;
  HIP_TRY(c, hipMalloc(&d_ctr, (size_t)n * 6u * sizeof(uint32_t)));
  if (hipMalloc(&d_out, (size_t)n * 6u * sizeof(double)) != hipSuccess) { dfree(d_ctr); return fail(c, EPV_ERR_HIP, "epv_philox_kat: allocation"); }
  hipError_t e = hipMemcpyAsync(d_ctr, counters, (size_t)n * 6u * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    epv_philox_kat_kernel<<<(n + 255u) / 256u, 256, 0, c->stream>>>((uint32_t)seed, (uint32_t)(seed >> 32), n, d_ctr, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * 6u * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  dfree(d_ctr); dfree(d_out);
  if (e != hipSuccess) return fail(c, EPV_ERR_HIP, std::string("epv_philox_kat: ") + hipGetErrorString(e));
  return EPV_OK;
}

// known-answer entry for the arithmetic under the MCMC kernels: one item = 4 doubles in, 6 out, evaluated
// by the project's own functions -- in a kernel of its own (one lane per item) and in this library's host
// pass of the same headers.  Ops 1 and 6 involve nojump_bound, which exists on the device only.
#define EPV_KAT_OPS 7u
EPV_DEV bool epv_math_kat_item(uint32_t op, const double *in, double *out) {
  double o[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool ok = true;
  switch (op) {
    case 0u: o[0] = epv_exp(in[0]); o[1] = epv_log(in[0]); break;
    case 2u: epv_seg_matrices(in[0], in[1], in[2], o); break;
    case 3u: { const double u = in[0], r = in[1]; o[0] = -epv_log(1.0 - u) / r; break; }
    case 4u: { const double u0 = in[0], trunc = in[1], r = in[2]; o[0] = -epv_log(1.0 - u0 * trunc) / r; break; }
    case 5u: o[0] = epv_u2d(epv_stat_fix(in[0], in[1])); break;
#if defined(__HIP_DEVICE_COMPILE__)
    case 1u: o[0] = nojump_bound(in[0]); break;
    case 6u: {
      const double u = in[0], T = in[1], r = in[2];
      o[0] = (1.0 - u < nojump_bound(T * r)) ? 1.0 : 0.0;
      o[1] = !(-epv_log(1.0 - u) / r < T) ? 1.0 : 0.0;
      break;
    }
#endif
    default: ok = false;
  }
  for (int i = 0; i < 6; ++i) out[i] = o[i];
  return ok;
}

__global__ void epv_math_kat_kernel(uint32_t op, uint32_t n, const double *in, double *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double x[4];
  for (int j = 0; j < 4; ++j) x[j] = in[4u * (size_t)i + j];
  epv_math_kat_item(op, x, out + 6u * (size_t)i);
}

EPV_API int epv_math_kat(epv_ctx *c, uint32_t op, uint32_t where, uint32_t n, const double *in, double *out) {
  if (!c || !in || !out || !n || n > (1u << 20) || op >= EPV_KAT_OPS || where > 1u) return EPV_ERR_ARG;
  if (where == 1u) {
    if (op == 1u || op == 6u) return EPV_ERR_ARG;   // the float bound has no host form
    for (uint32_t i = 0; i < n; ++i) epv_math_kat_item(op, in + 4u * (size_t)i, out + 6u * (size_t)i);
    return EPV_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  double *d_in = nullptr, *d_out = nullptr;
  HIP_TRY(c, hipMalloc(&d_in, (size_t)n * 4u * sizeof(double)));
  if (hipMalloc(&d_out, (size_t)n * 6u * sizeof(double)) != hipSuccess) { dfree(d_in); return fail(c, EPV_ERR_HIP, "epv_math_kat: allocation"); }
  hipError_t e = hipMemcpyAsync(d_in, in, (size_t)n * 4u * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    epv_math_kat_kernel<<<(n + 255u) / 256u, 256, 0, c->stream>>>(op, n, d_in, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)n * 6u * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  dfree(d_in); dfree(d_out);
  if (e != hipSuccess) return fail(c, EPV_ERR_HIP, std::string("epv_math_kat: ") + hipGetErrorString(e));
  return EPV_OK;
}

// known-answer entry for the three-way merge of a triple's jumps: item i = three paths of up to 8 jumps on
// one branch.  heads[i] = start states (bit 0 left, 1 middle, 2 right) | jump counts << 4, << 8, << 12;
// times[25 i + 8 col + k] = jump k of column col, times[25 i + 24] = the branch length.  A first kernel lays
// the times out as the jump store does (jump k of a path at j[k * n]); a second one runs merge3<Acc8> (the
// untouched form) and merge3_sel<AccLds> (heads loaded in one predicated batch first, as
// triple_llh_cached<NB > 0> does) on every item.  d_out / j_out[16 i + 8 form + ctx], form 0 = merge3.
// Like the two entries above this checks the function in a kernel of its own (one lane per item), not a
// call site inside the MCMC kernels.
#define EPV_MERGE_KAT_CAP 8u
__global__ void epv_merge_kat_layout_kernel(uint32_t n, const double *times, double *store) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (uint32_t q = 0; q < 3u * EPV_MERGE_KAT_CAP; ++q) store[(size_t)q * n + i] = times[25u * (size_t)i + q];
}

__global__ void __launch_bounds__(64) epv_merge_kat_kernel(uint32_t n, const uint32_t *heads, const double *times,
                                                           const double *store, double *d_out, uint32_t *j_out) {
  __shared__ double s_d[8 * 64];
  __shared__ uint32_t s_j[8 * 64];
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t h = heads[i];
  const double blen = times[25u * (size_t)i + 24u];
  PathRef P[3];
  for (uint32_t col = 0; col < 3u; ++col) {
    P[col].j = store + (size_t)col * EPV_MERGE_KAT_CAP * n + i;
    P[col].nj = (h >> (4u + 4u * col)) & 15u;
    P[col].init = (h >> col) & 1u;
  }
  Acc8 A8;
  acc_clear(A8);
  merge3(P[0], P[1], P[2], (uint64_t)n, blen, A8);
  AccLds AL;
  AL.d = s_d + threadIdx.x; AL.j = s_j + threadIdx.x; AL.stride = 64u;
  acc_clear(AL);
  const double tl = P[0].nj ? P[0].j[0] : EPV_INF, tm = P[1].nj ? P[1].j[0] : EPV_INF, tr = P[2].nj ? P[2].j[0] : EPV_INF;
  merge3_sel(P[0], P[1], P[2], tl, tm, tr, (uint64_t)n, blen, AL);
  for (int c = 0; c < 8; ++c) {
    d_out[16u * (size_t)i + c] = acc_d(A8, c); j_out[16u * (size_t)i + c] = acc_j(A8, c);
    d_out[16u * (size_t)i + 8u + c] = acc_d(AL, c); j_out[16u * (size_t)i + 8u + c] = acc_j(AL, c);
  }
}

EPV_API int epv_merge_kat(epv_ctx *c, uint32_t n, const uint32_t *heads, const double *times, double *d_out, uint32_t *j_out) {
  if (!c || !heads || !times || !d_out || !j_out || !n || n > (1u << 20)) return EPV_ERR_ARG;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t col = 0; col < 3u; ++col)
    {
      // (a finite time on every jump is what keeps a merge on paths that still have one: an item that
      // breaks it would walk off its column)
      const uint32_t nj = (heads[i] >> (4u + 4u * col)) & 15u;
      if (nj > EPV_MERGE_KAT_CAP) return EPV_ERR_ARG;
      for (uint32_t k = 0; k < nj; ++k)
        if (!(std::fabs(times[25u * (size_t)i + 8u * col + k]) < EPV_INF)) return EPV_ERR_ARG;
    }
  HIP_TRY(c, hipSetDevice(c->device));
  // one allocation: times [25 n] | store [24 n] | d_out [16 n] doubles, then heads [n] | j_out [16 n] words
  const size_t nd = (size_t)n * (25u + 24u + 16u), nw = (size_t)n * 17u;
  double *d_buf = nullptr;
  HIP_TRY(c, hipMalloc(&d_buf, nd * sizeof(double) + nw * sizeof(uint32_t)));
  double *d_times = d_buf, *d_store = d_buf + (size_t)n * 25u, *d_d = d_store + (size_t)n * 24u;
  uint32_t *d_heads = reinterpret_cast<uint32_t *>(d_buf + nd), *d_j = d_heads + n;
  hipError_t e = hipMemcpyAsync(d_times, times, (size_t)n * 25u * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_heads, heads, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    epv_merge_kat_layout_kernel<<<(n + 255u) / 256u, 256, 0, c->stream>>>(n, d_times, d_store);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    epv_merge_kat_kernel<<<(n + 63u) / 64u, 64, 0, c->stream>>>(n, d_heads, d_times, d_store, d_d, d_j);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(d_out, d_d, (size_t)n * 16u * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(j_out, d_j, (size_t)n * 16u * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  dfree(d_buf);
  if (e != hipSuccess) return fail(c, EPV_ERR_HIP, std::string("epv_merge_kat: ") + hipGetErrorString(e));
  return EPV_OK;
}

// known-answer entry for the trial evaluator of the end-conditioned sampler: item i = one segment and a first
// trial t0 (layout in include/epievo_mi355x.h).  One lane per item in waves of 64, so that the lanes of a wave
// mix flips with keepers and t == 1 with t >= 2 as the grouped search's do.  Five evaluations, in the form the
// fused bodies inline (plain multiplies, ONE first-draw block); the separate kernels' form is the parent's, and
// its two first-draw arms do not compile next to each other in one lane's straight-line code here (the
// compiler merges their tails and with them the scalar key chains of epv_philox.h):
//   0  scan_trial1 at t0                    1  run_trial at t0 on the GIVEN first draw u0 (no shortcut bounds)
//   2, 3, 4  scan_trials over W = 1, 4, 8 trials from t0
// w_out[20 i + 4 e ..] = outcome, winning trial, jumps, M;  d_out[11 i ..] = first_draw(t0), then the first two
// jump times of each evaluation.
template <bool ASM_MUL>
__device__ __forceinline__ void epv_trial_kat_form(uint32_t seed_lo, uint32_t seed_hi, const uint32_t *ci, const double *cd,
                                                   uint32_t *w_out, double *d_out) {
  const uint32_t site = ci[0], sweep = ci[1], node = ci[2], k = ci[3], t0 = ci[4], room = ci[5];
  const uint32_t a0 = ci[6] & 1u, end = (ci[6] >> 1) & 1u;
  const bool nielsen = (ci[6] >> 2) & 1u;
  const double T = cd[0], r0 = cd[1], r1 = cd[2], trunc = cd[3], u0 = cd[4], start = cd[5];
  d_out[0] = first_draw<ASM_MUL>(seed_lo, seed_hi, site, sweep, node, k, t0);
  for (uint32_t e = 0; e < 5u; ++e) {
    double jt[2] = {0.0, 0.0};
    uint32_t nj = 0u, tw = 0u, mm = 0u;
    int oc;
    if (e == 0u) {
      oc = scan_trial1<ASM_MUL>(seed_lo, seed_hi, site, sweep, node, k, t0, a0, end, T, r0, r1, trunc, room, jt, 1u, 2u, start,
                                nj, nielsen, &mm);
      tw = t0;
    } else if (e == 1u) {
      oc = run_trial<ASM_MUL>(seed_lo, seed_hi, site, sweep, node, k, t0, u0, a0, end, T, r0, r1, 0.0, 0.0, trunc, room, jt, 1u,
                              2u, start, nj, nielsen);
      tw = t0; mm = nj;
    } else {
      oc = scan_trials<ASM_MUL>(seed_lo, seed_hi, site, sweep, node, k, t0, e == 2u ? 1u : (e == 3u ? 4u : 8u), a0, end, T, r0,
                                r1, trunc, room, jt, 1u, 2u, start, tw, nj, nielsen, &mm);
    }
    w_out[4u * e] = (uint32_t)oc; w_out[4u * e + 1u] = tw; w_out[4u * e + 2u] = nj; w_out[4u * e + 3u] = mm;
    d_out[1u + 2u * e] = jt[0]; d_out[2u + 2u * e] = jt[1];
  }
}

__global__ void __launch_bounds__(64) epv_trial_kat_kernel(uint32_t seed_lo, uint32_t seed_hi, uint32_t n, const uint32_t *ci,
                                                           const double *cd, uint32_t *w_out, double *d_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  epv_trial_kat_form<false>(seed_lo, seed_hi, ci + 8u * (size_t)i, cd + 6u * (size_t)i, w_out + 20u * (size_t)i, d_out + 11u * (size_t)i);
}

EPV_API int epv_trial_kat(epv_ctx *c, uint64_t seed, uint32_t n, const uint32_t *items, const double *reals, uint32_t *w_out,
                          double *d_out) {
  if (!c || !items || !reals || !w_out || !d_out || !n || n > (1u << 16)) return EPV_ERR_ARG;
  for (uint32_t i = 0; i < n; ++i) {
    // (a trial index of 0 is no trial, and a rate or a length that is not positive and finite would keep a
    // lane in its hold-time loop)
    const uint32_t *w = items + 8u * (size_t)i;
    const double *r = reals + 6u * (size_t)i;
    if (w[4] == 0u || w[4] > 0x7fffffffu - 8u || w[2] > 4095u || w[3] > 4095u || w[6] > 7u) return EPV_ERR_ARG;
    if (!(r[0] > 0.0 && r[0] < EPV_INF && r[1] > 1e-3 && r[1] < EPV_INF && r[2] > 1e-3 && r[2] < EPV_INF)) return EPV_ERR_ARG;
    if (!(r[0] * (r[1] > r[2] ? r[1] : r[2]) <= 64.0)) return EPV_ERR_ARG;       // (bounds the jumps of a trial)
    if (!(r[3] >= 0.0 && r[3] < 1.0 && r[4] >= 0.0 && r[4] < 1.0 && std::fabs(r[5]) < EPV_INF)) return EPV_ERR_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // one allocation: reals [6 n] | d_out [11 n] doubles, then items [8 n] | w_out [20 n] words
  const size_t nd = (size_t)n * (6u + 11u), nw = (size_t)n * (8u + 20u);
  double *d_buf = nullptr;
  HIP_TRY(c, hipMalloc(&d_buf, nd * sizeof(double) + nw * sizeof(uint32_t)));
  double *d_reals = d_buf, *d_d = d_buf + (size_t)n * 6u;
  uint32_t *d_items = reinterpret_cast<uint32_t *>(d_buf + nd), *d_w = d_items + (size_t)n * 8u;
  hipError_t e = hipMemcpyAsync(d_reals, reals, (size_t)n * 6u * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_items, items, (size_t)n * 8u * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    epv_trial_kat_kernel<<<(n + 63u) / 64u, 64, 0, c->stream>>>((uint32_t)seed, (uint32_t)(seed >> 32), n, d_items, d_reals, d_w, d_d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(d_out, d_d, (size_t)n * 11u * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(w_out, d_w, (size_t)n * 20u * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  dfree(d_buf);
  if (e != hipSuccess) return fail(c, EPV_ERR_HIP, std::string("epv_trial_kat: ") + hipGetErrorString(e));
  return EPV_OK;
}

// known-answer entry for the direct end-conditioned sampler (epv_direct.h): one lane per item in waves of 64; item
// word 6 is the index of the segment's first draw (0 in every MCMC kernel), so that an item can cross trial words
__global__ void __launch_bounds__(64) epv_direct_kat_kernel(uint32_t seed_lo, uint32_t seed_hi, uint32_t n, const uint32_t *ci,
                                                            const double *cd, uint32_t *w_out, double *d_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  const uint32_t *w = ci + 8u * (size_t)i;
  const double *r = cd + 4u * (size_t)i;
  double jt[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  uint32_t nj = 0u, drawn = 0u, rounds = 0u;
  const int oc = run_direct((uint32_t)seed_lo, seed_hi, w[0], w[1], w[2], w[3], w[5] & 1u, (w[5] >> 1) & 1u, r[0], r[1], r[2],
                            w[4], jt, 1u, 8u, r[3], nj, drawn, rounds, w[6]);
  uint32_t *wo = w_out + 4u * (size_t)i;
  wo[0] = (uint32_t)oc; wo[1] = nj; wo[2] = drawn; wo[3] = rounds;
  for (uint32_t q = 0; q < 8u; ++q) d_out[8u * (size_t)i + q] = jt[q];
}

EPV_API int epv_direct_kat(epv_ctx *c, uint64_t seed, uint32_t n, const uint32_t *items, const double *reals, uint32_t *w_out,
                           double *d_out) {
  if (!c || !items || !reals || !w_out || !d_out || !n || n > (1u << 16)) return EPV_ERR_ARG;
  std::vector<uint32_t> it(items, items + 8u * (size_t)n);
  for (uint32_t i = 0; i < n; ++i) {
    // (the body returns whatever it is given; the checks keep an item what the restatement can follow)
    uint32_t *w = it.data() + 8u * (size_t)i;
    const double *r = reals + 4u * (size_t)i;
    if (w[2] > 4095u || w[3] > 4095u || w[5] > 3u) return EPV_ERR_ARG;
    // first draw index: 0, or the first half of a block (odd), far below the 32-bit trial word's end
    if (w[6] != 0u && ((w[6] & 1u) == 0u || w[6] > (1u << 24))) return EPV_ERR_ARG;
    if (!(r[0] > 0.0 && r[0] < EPV_INF && r[1] > 0.0 && r[1] < EPV_INF && r[2] > 0.0 && r[2] < EPV_INF && std::fabs(r[3]) < EPV_INF))
      return EPV_ERR_ARG;
    if (w[4] > 64u) w[4] = 64u;      // room: bounds the outer loop of a lane
  }
  HIP_TRY(c, hipSetDevice(c->device));
  // one allocation: reals [4 n] | d_out [8 n] doubles, then items [8 n] | w_out [4 n] words
  const size_t nd = (size_t)n * (4u + 8u), nw = (size_t)n * (8u + 4u);
  double *d_buf = nullptr;
  HIP_TRY(c, hipMalloc(&d_buf, nd * sizeof(double) + nw * sizeof(uint32_t)));
  double *d_reals = d_buf, *d_d = d_buf + (size_t)n * 4u;
  uint32_t *d_items = reinterpret_cast<uint32_t *>(d_buf + nd), *d_w = d_items + (size_t)n * 8u;
  hipError_t e = hipMemcpyAsync(d_reals, reals, (size_t)n * 4u * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_items, it.data(), (size_t)n * 8u * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    epv_direct_kat_kernel<<<(n + 63u) / 64u, 64, 0, c->stream>>>((uint32_t)seed, (uint32_t)(seed >> 32), n, d_items, d_reals, d_w, d_d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(d_out, d_d, (size_t)n * 8u * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(w_out, d_w, (size_t)n * 4u * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  dfree(d_buf);
  if (e != hipSuccess) return fail(c, EPV_ERR_HIP, std::string("epv_direct_kat: ") + hipGetErrorString(e));
  return EPV_OK;
}

EPV_API int epv_direct_giveups(epv_ctx *c, uint64_t *out) {
  if (!c || !out) return EPV_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long v = 0ull;
  HIP_TRY(c, hipMemcpyAsync(&v, c->d_counters + EPV_CNT_WORDS, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *out = v;
  return EPV_OK;
}

EPV_API int epv_set_unobserved(epv_ctx *c, const uint8_t *unobserved) {
  if (!c) return EPV_ERR_ARG;
  if (!c->have_paths) return fail(c, EPV_ERR_STATE, "paths must be resident before epv_set_unobserved");
  const uint32_t N = c->S.N;
  const uint64_t n = c->S.n;
  uint64_t cells = 0;
  uint32_t leaves = 0;
  for (uint32_t node = 1; node < N; ++node) {
    const bool leaf = c->subtree[node] == 1u;
    leaves += leaf ? 1u : 0u;
    if (!unobserved) continue;
    const uint8_t *row = unobserved + (uint64_t)(node - 1u) * n;
    uint64_t k = 0;
    for (uint64_t s = 0; s < n; ++s) k += row[s] != 0u;
    if (k && !leaf)
      return fail(c, EPV_ERR_ARG, "unobserved cells on branch " + std::to_string(node) +
                                      ", which does not end in a leaf (internal nodes are latent already)");
    cells += k;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (a queued phase may still read the old mask)
  dfree(c->d_unobs);
  c->unobs_cells = 0;
  if (!cells) return EPV_OK;   // nothing unobserved: today's kernels, no allocation
  // the layout of epv_unobserved: N words of row offsets, then one row of ceil(n / 32) words per leaf
  const uint64_t row = (n + 31u) / 32u;
  const uint64_t words = N + (uint64_t)leaves * row;
  if (words > 0xffffffffull) return fail(c, EPV_ERR_ARG, "mask of unobserved cells too large for 32-bit row offsets");
  std::vector<uint32_t> h(words, 0u);
  uint64_t at = N;
  for (uint32_t node = 1; node < N; ++node) {
    if (c->subtree[node] != 1u) continue;
    h[node] = (uint32_t)at;
    const uint8_t *src = unobserved + (uint64_t)(node - 1u) * n;
    for (uint64_t s = 0; s < n; ++s)
      if (src[s]) h[at + (s >> 5)] |= 1u << (s & 31u);
    at += row;
  }
  DevTmp<uint32_t> d;
  HIP_TRY(c, d.alloc(words));
  HIP_TRY(c, hipMemcpy(d.p, h.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
  c->d_unobs = d.release();
  c->unobs_cells = cells;
  return EPV_OK;
}

EPV_API int epv_unobserved_cells(epv_ctx *c, uint64_t *n_cells) {
  if (!c || !n_cells) return EPV_ERR_ARG;
  *n_cells = c->unobs_cells;
  return EPV_OK;
}

// fixed sites (epv_regions.h): a byte per local column.  The lists of the guard are built
// here, colour by colour ((g0 + site) % 3, as launch_phase colours the sites); columns 0 and n - 1 of a context are
// never updated and centre no triple, so they are kept in the mask and left out of the lists
EPV_API int epv_set_fixed_sites(epv_ctx *c, const uint8_t *mask) {
  if (!c) return EPV_ERR_ARG;
  if (!c->have_paths) return fail(c, EPV_ERR_STATE, "paths must be resident before epv_set_fixed_sites");
  const uint64_t n = c->S.n;
  bool any = false;
  for (uint64_t s = 0; mask && s < n && !any; ++s) any = mask[s] != 0;
  if (any)
    for (const SpanningLayer &sp : kSpanning)
      if (sp.L->on(c))
        return fail(c, EPV_ERR_STATE, std::string("epv_set_fixed_sites: ") + sp.L->name + " would count across fixed sites: " +
                                      "switch that layer off (" + sp.setter + " with 0) first");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  fixed_off(c);
  if (!any) return EPV_OK;   // nothing fixed: today's launches, no allocation
  std::vector<uint64_t> sites;
  uint64_t off[4] = {0, 0, 0, 0}, widest = 0;
  for (uint32_t colour = 0; colour < 3; ++colour) {
    for (uint64_t s = 1; s + 1 < n; ++s)
      if (mask[s] && (c->S.g0 + s) % 3u == colour) sites.push_back(s);
    off[colour + 1] = sites.size();
    widest = std::max<uint64_t>(widest, off[colour + 1] - off[colour]);
  }
  DevTmp<uint64_t> d_sites;
  DevTmp<uint32_t> d_sel;
  DevTmp<double> d_tri;
  if (!sites.empty()) {
    HIP_TRY(c, d_sites.alloc(sites.size()));
    HIP_TRY(c, d_sel.alloc(widest));
    HIP_TRY(c, d_tri.alloc(3u * widest));
    HIP_TRY(c, hipMemcpy(d_sites.p, sites.data(), sites.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
  }
  c->fx.mask.assign(mask, mask + n);
  c->fx.d_sites = d_sites.release();
  c->fx.save.sel = d_sel.release();
  c->fx.save.tri = d_tri.release();
  c->fx.save.cap = widest;
  for (int k = 0; k < 4; ++k) c->fx.off[k] = off[k];
  return EPV_OK;
}

// the fixed sites inside the owned range: what to take off the number of owned sites for an acceptance rate
EPV_API int epv_fixed_sites(epv_ctx *c, uint64_t *n_fixed_updatable) {
  if (!c || !n_fixed_updatable) return EPV_ERR_ARG;
  *n_fixed_updatable = 0;
  if (c->fx.mask.empty()) return EPV_OK;
  uint64_t lo = 0, hi = 0;
  owned_range(c, &lo, &hi);
  for (uint64_t s = lo; s <= hi && s < c->fx.mask.size(); ++s) *n_fixed_updatable += c->fx.mask[s] != 0;
  return EPV_OK;
}

EPV_API int epv_set_leaf_evidence(epv_ctx *c, const float *p_state1) {
  if (!c) return EPV_ERR_ARG;
  if (!c->have_paths) return fail(c, EPV_ERR_STATE, "paths must be resident before epv_set_leaf_evidence");
  const uint32_t N = c->S.N;
  const uint64_t n = c->S.n;
  uint64_t cells = 0;
  uint32_t leaves = 0;
  for (uint32_t node = 1; node < N; ++node) {
    const bool leaf = c->subtree[node] == 1u;
    leaves += leaf ? 1u : 0u;
    if (!p_state1) continue;
    const float *row = p_state1 + (uint64_t)(node - 1u) * n;
    for (uint64_t s = 0; s < n; ++s) {
      const float r = row[s];
      if (r != r) continue;   // NaN: no evidence
      if (!leaf)
        return fail(c, EPV_ERR_ARG, "leaf evidence on branch " + std::to_string(node) + " at site " + std::to_string(s) +
                                        ": the branch does not end in a leaf (internal nodes are latent already)");
      if (!(r >= 0.0f && r <= 1.0f))
        return fail(c, EPV_ERR_ARG, "leaf evidence on branch " + std::to_string(node) + " at site " + std::to_string(s) +
                                        " is " + std::to_string(r) + ": a probability in [0, 1] or NaN is needed");
      ++cells;
    }
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (a queued phase may still read the old table)
  dfree(c->d_evidence);
  c->evidence_cells = 0;
  if (!cells) return EPV_OK;   // no evidence: today's kernels, no allocation
  // the layout of epv_leaf_evidence: N words of row offsets, then one row of n float32 per leaf
  const uint64_t words = N + (uint64_t)leaves * n;
  if (words > 0xffffffffull) return fail(c, EPV_ERR_ARG, "table of leaf evidence too large for 32-bit row offsets");
  std::vector<uint32_t> h(words, 0u);
  uint64_t at = N;
  for (uint32_t node = 1; node < N; ++node) {
    if (c->subtree[node] != 1u) continue;
    h[node] = (uint32_t)at;
    std::memcpy(h.data() + at, p_state1 + (uint64_t)(node - 1u) * n, n * sizeof(float));
    at += n;
  }
  DevTmp<uint32_t> d;
  HIP_TRY(c, d.alloc(words));
  HIP_TRY(c, hipMemcpy(d.p, h.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice));
  c->d_evidence = d.release();
  c->evidence_cells = cells;
  return EPV_OK;
}

EPV_API int epv_leaf_evidence_cells(epv_ctx *c, uint64_t *n_cells) {
  if (!c || !n_cells) return EPV_ERR_ARG;
  *n_cells = c->evidence_cells;
  return EPV_OK;
}

EPV_API int epv_get_capacity(epv_ctx *c, uint32_t *capacity) {
  if (!c || !capacity || !c->have_paths) return EPV_ERR_ARG;
  *capacity = c->S.C;
  return EPV_OK;
}

EPV_API int epv_set_capacity(epv_ctx *c, uint32_t capacity) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (capacity < 1u) capacity = 1u;
  if (capacity > EPV_MAX_CAP) capacity = EPV_MAX_CAP;
  if (capacity == c->S.C) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t n = c->S.n, B = c->S.B, E = B * n;
  if (capacity < c->S.C) {
    // shrinking: every resident path (either buffer: a stale proposal is overwritten before
    // it is read, but keep the test simple) must fit
    std::vector<epv_meta_t> meta(2u * E);
    HIP_TRY(c, hipMemcpyAsync(meta.data(), c->S.meta, 2u * E * sizeof(epv_meta_t), hipMemcpyDeviceToHost, c->stream));
    std::vector<uint8_t> sel(n);
    HIP_TRY(c, hipMemcpyAsync(sel.data(), c->S.sel, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint64_t s = 0; s < n; ++s)
      for (uint64_t b = 0; b < B; ++b)
        if ((meta[((uint64_t)sel[s] * B + b) * n + s] & EPV_NJ_MASK) > capacity)
          return fail(c, EPV_ERR_CAPACITY, "a resident path has more jumps than the requested capacity");
  }
  DevTmp<double> nj;
  HIP_TRY(c, nj.alloc(2u * E * capacity));
  const uint32_t keep = std::min(capacity, c->S.C);
  // plane (buf, b) holds C rows of n doubles: rows 0..keep-1 move to the new stride
  for (uint64_t plane = 0; plane < 2u * B; ++plane)
    HIP_TRY(c, hipMemcpyAsync(nj.p + plane * capacity * n, c->S.jumps + plane * c->S.C * n,
                              (size_t)keep * n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  const uint32_t W = (2u * capacity + 1u + 63u) / 64u;
  DevTmp<uint64_t> ns;
  HIP_TRY(c, ns.alloc(B * c->S.phase_cap * W));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  (void)hipFree(c->S.jumps);
  (void)hipFree(c->S.prop_states);
  c->S.jumps = nj.release();
  c->S.prop_states = ns.release();
  c->S.C = capacity;
  c->S.W = W;
  return plan_kernels(c);
}

EPV_API int epv_init_paths_indep(epv_ctx *c, uint64_t n_sites, const uint8_t *root_states,
                                 const uint8_t *leaf_states, uint64_t seed, uint32_t capacity) {
  if (!c) return EPV_ERR_ARG;
  if (!c->have_tree || !c->have_model)
    return fail(c, EPV_ERR_STATE, "epv_set_tree and epv_set_model must come before epv_init_paths_indep");
  if (c->S.N != 2) return fail(c, EPV_ERR_ARG, "epv_init_paths_indep needs the two-node (single branch) tree");
  if (n_sites < 3 || !root_states || !leaf_states) return fail(c, EPV_ERR_ARG, "bad states");
  // device paths start as (init = root, no jumps)
  std::vector<uint64_t> off(n_sites + 1, 0);
  double dummy = 0.0;
  int rc = epv_upload_paths(c, n_sites, root_states, off.data(), &dummy, capacity ? capacity : 32u, 0);
  if (rc) return rc;
  DevTmp<uint8_t> leaf_tmp;
  HIP_TRY(c, leaf_tmp.alloc(n_sites));
  uint8_t *d_leaf = leaf_tmp.p;
  HIP_TRY(c, hipMemcpyAsync(d_leaf, leaf_states, n_sites, hipMemcpyHostToDevice, c->stream));
  const uint64_t first = 1, last = n_sites - 2;
  const uint64_t threads = (last - first + 1u + 2u) / 3u;
  const unsigned blocks = (unsigned)((threads + 255u) / 256u);
  for (uint32_t colour = 0; colour < 3; ++colour) {
    const uint64_t s0 = first + ((colour + 3u - (uint32_t)((c->S.g0 + first) % 3u)) % 3u);
    // 64-lane blocks like epv_mh_propose_kernel: the per-shard task regions are sized for them
    hipLaunchKernelGGL(epv_init_tasks_kernel, dim3((unsigned)((threads + 63u) / 64u)), dim3(64), 0, c->stream,
                       c->S, colour, first, last, d_leaf, c->d_counters);
    const uint64_t per_shard = threads / EPV_SHARDS + 256u;
    const uint32_t tpw = 32u;
    const uint64_t jb = std::min<uint64_t>((per_shard + 4u * tpw - 1u) / (4u * tpw), 256u);
    hipLaunchKernelGGL(epv_mh_jumps_kernel, dim3((unsigned)jb, EPV_SHARDS), dim3(256), const_lds_bytes(c->S.N),
                       c->stream, c->S, (uint32_t)seed, (uint32_t)(seed >> 32), EPV_INIT_SWEEP,
                       tpw, s0, 0.0, 0.0, c->d_counters);
    hipLaunchKernelGGL(epv_init_commit_kernel, dim3(blocks), dim3(256), 0, c->stream, c->S, colour, first,
                       last, c->d_counters);
  }
  hipLaunchKernelGGL(epv_init_flip_kernel, dim3((unsigned)((last - first + 256u) / 256u)), dim3(256), 0,
                     c->stream, c->S, first, last);
  hipLaunchKernelGGL(epv_init_ends_kernel, dim3(1), dim3(64), 0, c->stream, c->S, d_leaf, (uint32_t)seed,
                     (uint32_t)(seed >> 32), c->blen[1]);
  HIP_TRY(c, hipGetLastError());
  return finish_mcmc(c, nullptr, 0);  // synchronises (d_leaf is released afterwards); reports overflow
}

// ---------------------------------------------------------------------------------------
//  site-independent model (IndepSite.cpp), used by epievo_initialization
// ---------------------------------------------------------------------------------------
namespace {
// continuous_time_trans_prob_mat + expectation_J/D (ContinuousTimeMarkovModel.cpp:143-226)
// for every branch, with epv_exp so that the values equal the oracle's parallel rung
int upload_indep_consts(epv_ctx *c, const double *rates) {
  if (!(rates[0] > 0.0) || !(rates[1] > 0.0)) return fail(c, EPV_ERR_ARG, "indep rates must be positive");
  std::vector<EpvIndepConst> k(c->S.N);
  const double r0 = rates[0], r1 = rates[1];
  for (uint32_t node = 1; node < c->S.N; ++node) {
    const double T = c->blen[node];
    EpvIndepConst &q = k[node];
    {
      const double h = 1.0 / epv_exp(T * (r0 + r1));
      const double denom = r0 + r1;
      q.P[0] = (r0 * h + r1) / denom;
      q.P[1] = 1.0 - q.P[0];
      q.P[3] = (r0 + r1 * h) / denom;
      q.P[2] = 1.0 - q.P[3];
    }
    const double s = r0 + r1, p = r0 * r1, d = r1 - r0;
    const double e = epv_exp(-s * T);
    const double C1 = d * (1 - e) / s;
    q.J0[0] = p * (T * (r1 - r0 * e) - C1) / (s * (r1 + r0 * e));
    q.J1[0] = q.J0[0];
    q.J0[3] = p * (T * (r0 - r1 * e) + C1) / (s * (r0 + r1 * e));
    q.J1[3] = q.J0[3];
    const double C2 = p * T * (1 + e) / (s * (1 - e));
    const double C3 = (r0 * r0 + r1 * r1) / (s * s);
    const double C4 = (2 * p) / (s * s);
    q.J0[1] = C2 + C3; q.J1[1] = C2 - C4; q.J0[2] = q.J1[1]; q.J1[2] = q.J0[1];
    const double r00 = r0 * r0, r11 = r1 * r1;
    const double E1 = 2 * p * (1 - e) / s;
    q.D0[0] = ((r11 + r00 * e) * T + E1) / (s * (r1 + r0 * e));
    q.D1[0] = T - q.D0[0];
    q.D1[3] = ((r00 + r11 * e) * T + E1) / (s * (r0 + r1 * e));
    q.D0[3] = T - q.D1[3];
    const double E2 = (p - r00) * (1 - e) / s;
    q.D1[1] = ((r00 - p * e) * T + E2) / (s * (r0 - r0 * e));
    q.D0[1] = T - q.D1[1];
    const double E3 = (p - r11) * (1 - e) / s;
    q.D0[2] = ((r11 - p * e) * T + E3) / (s * (r1 - r1 * e));
    q.D1[2] = T - q.D0[2];
  }
  if (!c->d_indep) HIP_TRY(c, hipMalloc(&c->d_indep, sizeof(EpvIndepConst) * c->S.N));
  HIP_TRY(c, hipMemcpy(c->d_indep, k.data(), sizeof(EpvIndepConst) * c->S.N, hipMemcpyHostToDevice));
  return EPV_OK;
}

// launch shape of the kernels that keep a per-node table of 5 doubles per lane in LDS: 256-lane blocks when
// it fits, 64-lane blocks for large trees
void indep_stats_shape(const epv_ctx *c, uint32_t &threads, size_t &lds) {
  threads = 256u;
  lds = (size_t)c->S.N * threads * 5u * sizeof(double);
  if (lds > 60u * 1024u) { threads = 64u; lds = (size_t)c->S.N * threads * 5u * sizeof(double); }
}

int indep_stats(epv_ctx *c, const double *rates, uint32_t what, double *J, double *D) {
  const uint32_t B = c->S.B, V16 = ((B * 4u + 15u) / 16u) * 16u;
  uint32_t threads = 0;
  size_t lds = 0;
  indep_stats_shape(c, threads, lds);
  const uint64_t nb = (c->S.n + threads - 1u) / threads;
  // the tree-reduction buffers are shared with the 8-context statistics but sized for THIS
  // launch shape: nb rows of V16 doubles at level 0, ceil(nb/256) rows at level 1
  int rc = ensure_partial_doubles(c, nb * V16, ((nb + 255u) / 256u) * V16);
  if (rc) return rc;
  if (lds > 150u * 1024u) return fail(c, EPV_ERR_ARG, "tree too large for the site-independent kernels");
  // the leaf vector: the table instantiation only while the context holds a flagged
  // or non-NaN cell and the call reads leaf data; otherwise the kernel a context without tables always ran
  const bool tables = what == 0u && (c->d_evidence || c->d_unobs);
  typedef const uint32_t *M;
  if (lds > 60u * 1024u &&
      hipFuncSetAttribute(tables ? reinterpret_cast<const void *>(epv_indep_stats_kernel<EPV_LEAF_EVIDENCE, M, M>)
                                 : reinterpret_cast<const void *>(epv_indep_stats_kernel<EPV_LEAF_DATA>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail(c, EPV_ERR_HIP, "cannot raise the dynamic LDS limit");
  double pi_0 = 0.0;
  if (what == 0u) pi_0 = rates[1] / (rates[0] + rates[1]);
  if (tables)
    hipLaunchKernelGGL((epv_indep_stats_kernel<EPV_LEAF_EVIDENCE, M, M>), dim3((unsigned)nb), dim3(threads), lds,
                       c->stream, c->S, c->d_indep, pi_0, what, V16, c->d_partial[0], (M)c->d_evidence, (M)c->d_unobs);
  else
    hipLaunchKernelGGL((epv_indep_stats_kernel<EPV_LEAF_DATA>), dim3((unsigned)nb), dim3(threads), lds, c->stream,
                       c->S, c->d_indep, pi_0, what, V16, c->d_partial[0]);
  uint64_t m = nb;
  int cur = 0;
  while (m > 1) {
    const uint64_t mb = (m + 255u) / 256u;
    hipLaunchKernelGGL(epv_tree_reduce_kernel, dim3((unsigned)mb, V16 / 16u), dim3(256), 0, c->stream,
                       c->d_partial[cur], m, V16, c->d_partial[cur ^ 1]);
    m = mb;
    cur ^= 1;
  }
  HIP_TRY(c, hipGetLastError());
  std::vector<double> v(V16);
  HIP_TRY(c, hipMemcpyAsync(v.data(), c->d_partial[cur], V16 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (uint32_t b = 0; b < B; ++b) {
    J[b * 2 + 0] = v[b * 4 + 0]; J[b * 2 + 1] = v[b * 4 + 1];
    D[b * 2 + 0] = v[b * 4 + 2]; D[b * 2 + 1] = v[b * 4 + 3];
  }
  return EPV_OK;
}
}  // namespace

EPV_API int epv_indep_expectation(epv_ctx *c, const double *rates, double *J, double *D) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (!rates || !J || !D) return fail(c, EPV_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = upload_indep_consts(c, rates))) return rc;
  return indep_stats(c, rates, 0u, J, D);
}

EPV_API int epv_indep_sufficient_statistics(epv_ctx *c, double *J, double *D) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (!J || !D) return fail(c, EPV_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->device));
  const double one[2] = {1.0, 1.0};
  if ((rc = upload_indep_consts(c, one))) return rc;   // constants unused by the counting mode
  if ((rc = indep_stats(c, one, 1u, J, D))) return rc;
  for (uint32_t i = 0; i < 2u * c->S.B; ++i) {   // averages over the sites (IndepSite.cpp:291-295)
    J[i] /= (double)c->S.n;
    D[i] /= (double)c->S.n;
  }
  return EPV_OK;
}

EPV_API int epv_indep_node_posterior(epv_ctx *c, const double *rates, double *p_state1) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (!rates || !p_state1) return fail(c, EPV_ERR_ARG, "null argument");
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = upload_indep_consts(c, rates))) return rc;
  uint32_t threads = 0;
  size_t lds = 0;
  indep_stats_shape(c, threads, lds);
  if (lds > 150u * 1024u) return fail(c, EPV_ERR_ARG, "tree too large for the site-independent kernels");
  if (lds > 60u * 1024u &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(epv_indep_posterior_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail(c, EPV_ERR_HIP, "cannot raise the dynamic LDS limit");
  // the read-out is staged on the device, [N][n] doubles
  const uint64_t cells = (uint64_t)c->S.N * c->S.n;
  const double need = 8.0 * (double)cells;
  bool fits = false;
  double free_b = 0.0;
  if ((rc = device_room(c, need, &fits, &free_b))) return rc;
  if (!fits) {
    char buf[320];
    std::snprintf(buf, sizeof buf, "node posterior needs %.3g GB of device memory (8 B x %u nodes x %llu sites); "
                  "%.3g GB are free", need / 1e9, c->S.N, (unsigned long long)c->S.n, free_b / 1e9);
    return fail(c, EPV_ERR_ARG, buf);
  }
  DevTmp<double> out;
  HIP_TRY(c, out.alloc(cells));
  const uint64_t nb = (c->S.n + threads - 1u) / threads;
  hipLaunchKernelGGL(epv_indep_posterior_kernel, dim3((unsigned)nb), dim3(threads), lds, c->stream, c->S, c->d_indep,
                     rates[1] / (rates[0] + rates[1]), (const uint32_t *)c->d_evidence, (const uint32_t *)c->d_unobs,
                     out.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(p_state1, out.p, cells * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}

EPV_API int epv_indep_update_paths(epv_ctx *c, const double *rates, uint64_t seed, uint32_t sweep) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (!rates) return fail(c, EPV_ERR_ARG, "null argument");
  if (c->S.g0 != 0) return fail(c, EPV_ERR_ARG, "epv_indep_update_paths works on an unsharded genome");
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = upload_indep_consts(c, rates))) return rc;
  const uint64_t first = 0, last = c->S.n - 1;
  const uint64_t threads = (last - first + 1u + 2u) / 3u;
  const size_t lds = (size_t)c->S.N * 64u * 4u * sizeof(double);
  if (lds > 150u * 1024u) return fail(c, EPV_ERR_ARG, "tree too large for the site-independent kernels");
  const bool tables = c->d_evidence || c->d_unobs;   // the leaf vector: as in indep_stats
  typedef const uint32_t *M;
  if (lds > 60u * 1024u &&
      hipFuncSetAttribute(tables ? reinterpret_cast<const void *>(epv_indep_propose_kernel<EPV_LEAF_EVIDENCE, M, M>)
                                 : reinterpret_cast<const void *>(epv_indep_propose_kernel<EPV_LEAF_DATA>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail(c, EPV_ERR_HIP, "cannot raise the dynamic LDS limit");
  for (uint32_t colour = 0; colour < 3; ++colour) {
    const uint64_t s0 = first + ((colour + 3u - (uint32_t)((c->S.g0 + first) % 3u)) % 3u);
    const uint64_t blocks = (threads + 63u) / 64u;
    if (tables)
      hipLaunchKernelGGL((epv_indep_propose_kernel<EPV_LEAF_EVIDENCE, M, M>), dim3((unsigned)blocks), dim3(64), lds,
                         c->stream, c->S, c->d_indep, rates[0], rates[1], colour, first, last, (uint32_t)seed,
                         (uint32_t)(seed >> 32), sweep, c->d_counters, (M)c->d_evidence, (M)c->d_unobs);
    else
      hipLaunchKernelGGL((epv_indep_propose_kernel<EPV_LEAF_DATA>), dim3((unsigned)blocks), dim3(64), lds, c->stream,
                         c->S, c->d_indep, rates[0], rates[1], colour, first, last, (uint32_t)seed,
                         (uint32_t)(seed >> 32), sweep, c->d_counters);
    const uint64_t max_tasks = blocks / EPV_SHARDS * 64u * c->S.B + 64u * c->S.B;
    const uint32_t tpw = 32u;
    const uint64_t jb = std::min<uint64_t>((max_tasks / 4u + 4u * tpw - 1u) / (4u * tpw) + 1u, 256u);
    hipLaunchKernelGGL(epv_mh_jumps_kernel, dim3((unsigned)jb, EPV_SHARDS), dim3(256), const_lds_bytes(c->S.N),
                       c->stream, c->S, (uint32_t)seed, (uint32_t)(seed >> 32), sweep, tpw, s0, rates[0],
                       rates[1], c->d_counters);
    hipLaunchKernelGGL(epv_indep_commit_kernel, dim3((unsigned)((threads + 255u) / 256u)), dim3(256), 0,
                       c->stream, c->S, colour, first, last, c->d_counters);
  }
  HIP_TRY(c, hipGetLastError());
  c->have_reset = false;
  return finish_mcmc(c, nullptr, 0);
}

EPV_API int epv_set_global_length(epv_ctx *c, uint64_t n_global) {
  if (!c || !c->have_paths) return EPV_ERR_ARG;
  if (n_global < c->S.g0 + c->S.n) return fail(c, EPV_ERR_ARG, "n_global smaller than the shard");
  c->S.n_global = n_global;
  return EPV_OK;
}

EPV_API int epv_set_update_range(epv_ctx *c, uint64_t first, uint64_t last) {
  if (!c || !c->have_paths) return EPV_ERR_ARG;
  if (first < 1 || last > c->S.n - 2 || first > last) return fail(c, EPV_ERR_ARG, "bad update range");
  if (c->S.g0 + first > 1 && first < 2) return fail(c, EPV_ERR_ARG, "shard needs a 2-site left halo");
  if (c->S.g0 + last < c->S.n_global - 2 && last > c->S.n - 3)
    return fail(c, EPV_ERR_ARG, "shard needs a 2-site right halo");
  c->first = first;
  c->last = last;
  c->halo_mode = false;
  return EPV_OK;
}

EPV_API int epv_set_halo(epv_ctx *c, uint64_t left, uint64_t right) {
  if (!c || !c->have_paths) return EPV_ERR_ARG;
  if ((left && left < 2) || (right && right < 2) || left + right + 1 > c->S.n)
    return fail(c, EPV_ERR_ARG, "halo blocks must be 0 or >= 2 columns and leave owned columns");
  if (!left && c->S.g0 != 0) return fail(c, EPV_ERR_ARG, "a shard that does not start the genome needs a left halo");
  if (!right && c->S.g0 + c->S.n != c->S.n_global)
    return fail(c, EPV_ERR_ARG, "a shard that does not end the genome needs a right halo");
  c->halo_left = left;
  c->halo_right = right;
  c->halo_mode = true;
  c->phases_used = 0;
  return EPV_OK;
}

EPV_API int epv_halo_phases_left(epv_ctx *c, uint64_t *phases) {
  if (!c || !phases || !c->have_paths) return EPV_ERR_ARG;
  if (!c->halo_mode || (!c->halo_left && !c->halo_right)) { *phases = ~0ull; return EPV_OK; }
  uint64_t h = ~0ull;
  if (c->halo_left) h = std::min(h, c->halo_left);
  if (c->halo_right) h = std::min(h, c->halo_right);
  const uint64_t total = h / 2u;  // phase p needs 2(p+1) <= halo
  *phases = total > c->phases_used ? total - c->phases_used : 0;
  return EPV_OK;
}

// the reset's launches without waiting for them: the MCMC calls that follow sit behind them on the
// context's stream (an EM driver goes from reset straight into run_mcmc: the device need not idle
// while the host finds that out)
EPV_API int epv_reset_async(epv_ctx *c) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->d_segtab) HIP_TRY(c, hipMalloc(&c->d_segtab, (size_t)4095u * 4u * 6u * sizeof(double)));
  hipLaunchKernelGGL(epv_reset_kernel, dim3((unsigned)((c->S.n + 255u) / 256u)), dim3(256),
                     const_lds_bytes(c->S.N), c->stream, c->S);
  // the single-segment matrices of every (branch, neighbour context): model and branch lengths
  // are fixed until the next reset
  hipLaunchKernelGGL(epv_segtab_kernel, dim3((c->S.B * 4u + 63u) / 64u), dim3(64), 0, c->stream, c->S, c->d_segtab);
  HIP_TRY(c, hipGetLastError());
  c->have_reset = true;
  return EPV_OK;
}

EPV_API int epv_reset(epv_ctx *c) {
  int rc = epv_reset_async(c);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}

static int finish_mcmc(epv_ctx *c, uint64_t *n_accepted, uint64_t acc_base) {
  unsigned long long cnt[EPV_CNT_N];
  int rc = read_counters(c, cnt);
  if (rc) return rc;
  if (n_accepted) *n_accepted = cnt[EPV_CNT_ACCEPT] - acc_base;
  const uint64_t new_ovf = cnt[EPV_CNT_OVERFLOW] - c->tot_overflow;
  c->tot_overflow = cnt[EPV_CNT_OVERFLOW];
  c->tot_coop = cnt[EPV_CNT_COOP];
  if (new_ovf) {
    char buf[160];
    std::snprintf(buf, sizeof buf,
                  "%llu proposals needed more than %u jumps on a branch and were rejected; "
                  "re-upload with a larger capacity",
                  (unsigned long long)new_ovf, c->S.C);
    return fail(c, EPV_ERR_CAPACITY, buf);
  }
  return EPV_OK;
}

// the accept counters of this moment of the stream, kept on the device; finish_mcmc_snapshot reads them
// back together with the final ones -- no host synchronisation in the middle of a run
static int snapshot_counters(epv_ctx *c) {
  HIP_TRY(c, hipMemcpyAsync(c->d_cnt_snap, c->d_counters, sizeof(unsigned long long) * EPV_CNT_WORDS,
                            hipMemcpyDeviceToDevice, c->stream));
  return EPV_OK;
}
static int finish_mcmc_snapshot(epv_ctx *c, uint64_t *n_accepted) {
  HIP_TRY(c, hipMemcpyAsync(c->h_cnt_snap, c->d_cnt_snap, sizeof(unsigned long long) * EPV_CNT_WORDS,
                            hipMemcpyDeviceToHost, c->stream));
  uint64_t total = 0;
  int rc = finish_mcmc(c, &total, 0);      // synchronises the stream
  uint64_t base = 0;
  for (uint32_t sh = 0; sh < EPV_SHARDS; ++sh) base += c->h_cnt_snap[EPV_CNT_IDX(EPV_CNT_ACCEPT, sh)];
  if (n_accepted) *n_accepted = total - base;
  return rc;
}

static int current_accepts(epv_ctx *c, uint64_t *out) {
  unsigned long long cnt[EPV_CNT_N];
  int rc = read_counters(c, cnt);
  if (rc) return rc;
  *out = cnt[EPV_CNT_ACCEPT];
  return EPV_OK;
}

EPV_API int epv_sweep_phase(epv_ctx *c, int colour, uint64_t seed, uint32_t sweep,
                            uint64_t *n_accepted) {
  int rc = check_ready(c, true);
  if (rc) return rc;
  if (colour < 0 || colour > 2) return fail(c, EPV_ERR_ARG, "colour must be 0, 1 or 2");
  HIP_TRY(c, hipSetDevice(c->device));
  uint64_t base = 0;
  if ((rc = current_accepts(c, &base))) return rc;
  if ((rc = launch_phase(c, colour, seed, sweep))) return rc;
  return finish_mcmc(c, n_accepted, base);
}

EPV_API int epv_sweep(epv_ctx *c, uint64_t n_sweeps, uint64_t seed, uint32_t sweep_base,
                      uint64_t *n_accepted) {
  int rc = check_ready(c, true);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  uint64_t base = 0;
  if ((rc = current_accepts(c, &base))) return rc;
  for (uint64_t w = 0; w < n_sweeps; ++w) {
    for (int colour = 0; colour < 3; ++colour)
      if ((rc = launch_phase(c, colour, seed, sweep_base + (uint32_t)w))) return rc;
    ++c->n_sweeps;
  }
  return finish_mcmc(c, n_accepted, base);
}

// burn_in sweeps, then batch x {sweep; stat(w); one sample of every summary layer that is on, in the order of
// kLayers}: the chain of epv_run_mcmc_sums and epv_run_mcmc_counts.  A layer with a begin() sees the state after
// burn-in first.  stat(w) launches the statistics of batch
// sweep w; the accept counters are snapshot where the batch sweeps begin (finish_mcmc_snapshot)
template <class Stat>
static int run_chain(epv_ctx *c, uint64_t burn_in, uint64_t batch, uint64_t seed, uint32_t sweep_base, Stat stat) {
  int rc = EPV_OK;
  for (const Layer *L : kLayers)   // (the caps before any sweep: the chain is not cut short)
    if (L->on(c) && ((rc = L->ensure(c)) || (rc = L->check_cap(c, batch)))) return rc;
  uint32_t sweep = sweep_base;
  for (uint64_t w = 0; w < burn_in; ++w, ++sweep) {
    for (int colour = 0; colour < 3; ++colour)
      if ((rc = launch_phase(c, colour, seed, sweep))) return rc;
    ++c->n_sweeps;
  }
  if ((rc = snapshot_counters(c))) return rc;
  for (const Layer *L : kLayers)   // (the opening state of what is joint across samples)
    if (L->begin && L->on(c) && (rc = L->begin(c))) return rc;
  for (uint64_t w = 0; w < batch && !rc; ++w, ++sweep) {
    for (int colour = 0; colour < 3 && !rc; ++colour) rc = launch_phase(c, colour, seed, sweep);
    if (rc) break;
    ++c->n_sweeps;
    if ((rc = stat(w))) break;
    for (const Layer *L : kLayers)
      if (L->on(c) && (rc = L->launch(c))) break;
  }
  mixing_close_run(c);   // nothing links across two calls: parameters and branch lengths may change between them
  if (rc) return rc;
  HIP_TRY(c, hipGetLastError());
  return EPV_OK;
}

EPV_API int epv_run_mcmc_sums(epv_ctx *c, uint64_t burn_in, uint64_t batch, uint64_t seed,
                              uint32_t sweep_base, int average, double *J, double *D,
                              uint64_t *n_accepted) {
  int rc = check_ready(c, true);
  if (rc) return rc;
  if (!J || !D || batch == 0) return fail(c, EPV_ERR_ARG, "bad run_mcmc arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = ensure_sweep_tot(c, batch))) return rc;
  if ((rc = ensure_partials(c))) return rc;      // (allocations synchronise: before the chain)
  rc = run_chain(c, burn_in, batch, seed, sweep_base, [c](uint64_t w) { return launch_suffstats(c, w); });
  if (rc) return rc;
  rc = finish_mcmc_snapshot(c, n_accepted);  // synchronises the stream
  const int src = finish_stats(c, batch, average, J, D);
  return rc ? rc : src;
}

// what epv_run_mcmc_counts hands back, fetched with ONE wait: the accept counters as they stood when the batch
// sweeps began, the final counters and the sweep totals leave as three stream-ordered copies into pinned memory
static int finish_counts(epv_ctx *c, uint64_t batch, int64_t *counts, uint64_t *n_accepted) {
  const uint64_t words = batch * c->S.B * 16u;
  if (words > c->h_tot_cap) {
    if (c->h_tot) HIP_TRY(c, hipHostFree(c->h_tot));
    c->h_tot = nullptr;
    c->h_tot_cap = 0;
    HIP_TRY(c, hipHostMalloc(&c->h_tot, words * sizeof(long long)));
    c->h_tot_cap = words;
  }
  HIP_TRY(c, hipMemcpyAsync(c->h_cnt_snap, c->d_cnt_snap, sizeof(unsigned long long) * EPV_CNT_WORDS,
                            hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->h_tot, c->d_sweep_tot, words * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  uint64_t total = 0;
  const int rc = finish_mcmc(c, &total, 0);      // the final counters; synchronises the stream
  if (rc && rc != EPV_ERR_CAPACITY) return rc;   // (an overflow leaves complete outputs)
  uint64_t base = 0;
  for (uint32_t sh = 0; sh < EPV_SHARDS; ++sh) base += c->h_cnt_snap[EPV_CNT_IDX(EPV_CNT_ACCEPT, sh)];
  if (n_accepted) *n_accepted = total - base;
  std::memcpy(counts, c->h_tot, words * sizeof(long long));
  return rc;
}

// ---- a context that shares its GPU with others (the sharded drivers).  Its statistics run as
// one-wave blocks (they fit into the LDS the colour phases leave free); the waves add into EPV_STATW_ROWS
// rows per sweep of d_partial[0] ([w][row][16 B], zeroed first; a 256-site block adds into row block % rows,
// so a word takes a few dozen adds per launch, not thousands), and one reduction after the last sweep leaves
// the per-sweep totals in d_sweep_tot
EPV_API int epv_run_mcmc_counts(epv_ctx *c, uint64_t burn_in, uint64_t batch, uint64_t seed, uint32_t sweep_base,
                                int64_t *counts, uint64_t *n_accepted) {
  int rc = check_ready(c, true);
  if (rc) return rc;
  if (!counts || batch == 0) return fail(c, EPV_ERR_ARG, "bad run_mcmc_counts arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t V = c->S.B * 16u;
  uint64_t own_lo = 0, own_hi = 0;
  owned_range(c, &own_lo, &own_hi);
  const uint64_t blk_lo = own_lo / 256u, n_own = own_hi / 256u - blk_lo + 1u;
  if ((rc = ensure_stat_scale(c))) return rc;
  if ((rc = ensure_sweep_tot(c, batch))) return rc;
  const uint32_t n_rows = (uint32_t)std::min<uint64_t>(n_own, EPV_STATW_ROWS);
  if ((rc = ensure_partials(c, batch * n_rows))) return rc;
  unsigned long long *rows = (unsigned long long *)c->d_partial[0];
  HIP_TRY(c, hipMemsetAsync(rows, 0, batch * n_rows * V * sizeof(unsigned long long), c->stream));
  rc = run_chain(c, burn_in, batch, seed, sweep_base, [&](uint64_t w) {
    hipLaunchKernelGGL(epv_suffstat_wave_kernel, dim3((unsigned)(n_own * 4u), (c->S.B + EPV_STATW_BCH - 1u) / EPV_STATW_BCH),
                       dim3(64), 0, c->stream, c->S, own_lo, own_hi, blk_lo, c->d_statscale, rows + w * n_rows * V, n_rows);
    launch_fixed_unstat(c, own_lo, own_hi, rows + w * n_rows * V);   // (off row 0 of the sweep: the rows are summed)
    return EPV_OK;
  });
  if (rc) return rc;
  if ((rc = reduce_blocks_to_tot(c, rows, n_rows, batch, 0u))) return rc;   // (at most 1024 rows: one stage)
  return finish_counts(c, batch, counts, n_accepted);
}

EPV_API int epv_counts_to_stats(epv_ctx *c, const int64_t *counts, uint64_t batch, int average, double *J, double *D) {
  if (!c || !counts || !J || !D || !batch) return EPV_ERR_ARG;
  if (!c->have_tree) return fail(c, EPV_ERR_STATE, "epv_set_tree must come first");
  HIP_TRY(c, hipSetDevice(c->device));
  const int rc = ensure_stat_scale(c);     // k_b depends on the genome length and the branch lengths
  if (rc) return rc;
  counts_to_stats(c, counts, batch, average, J, D);
  return EPV_OK;
}

// device buffers on the context's GPU for the sharded drivers: the halo columns and the all-gather
// pieces they hand to RCCL, and small host <-> device copies into and out of them (e.g. the
// statistics piece with its tail, so that ONE all-gather carries everything)
EPV_API int epv_dev_alloc(epv_ctx *c, uint64_t bytes, void **p) {
  if (!c || !p || !bytes) return EPV_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMalloc(p, bytes));
  HIP_TRY(c, hipMemset(*p, 0, bytes));
  HIP_TRY(c, hipDeviceSynchronize());   // the contexts' streams do not wait for the null stream
  return EPV_OK;
}
EPV_API int epv_dev_write(epv_ctx *c, void *d_dst, const void *src, uint64_t bytes) {
  if (!c || !d_dst || !src) return EPV_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
  return EPV_OK;
}
EPV_API int epv_dev_read(epv_ctx *c, void *dst, const void *d_src, uint64_t bytes) {
  if (!c || !dst || !d_src) return EPV_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
  return EPV_OK;
}
EPV_API int epv_dev_free(epv_ctx *c, void *p) {
  if (!c) return EPV_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  if (p) HIP_TRY(c, hipFree(p));
  return EPV_OK;
}

EPV_API int epv_run_mcmc(epv_ctx *c, uint64_t burn_in, uint64_t batch, uint64_t seed,
                         uint32_t sweep_base, double *J, double *D, uint64_t *n_accepted) {
  return epv_run_mcmc_sums(c, burn_in, batch, seed, sweep_base, 1, J, D, n_accepted);
}

EPV_API int epv_get_sufficient_statistics(epv_ctx *c, double *J, double *D) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = launch_suffstats(c, 0u))) return rc;
  return finish_stats(c, 1u, 0, J, D);
}

EPV_API int epv_scale_jump_times(epv_ctx *c, const double *new_branches) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<double> scale(c->S.N, 1.0);
  for (uint32_t b = 1; b < c->S.N; ++b) {
    if (!(new_branches[b] > 0.0)) return fail(c, EPV_ERR_ARG, "branch lengths must be positive");
    scale[b] = new_branches[b] / c->blen[b];  // ParamEstimation.cpp:372
  }
  HIP_TRY(c, hipMemcpyAsync(c->d_scale, scale.data(), sizeof(double) * c->S.N, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(epv_scale_kernel, dim3((unsigned)((c->S.n + 255u) / 256u)), dim3(256), 0,
                     c->stream, c->S, c->d_scale);
  mixing_close_run(c);   // (every jump time changed: not a move of the chain)
  HIP_TRY(c, hipGetLastError());
  for (uint32_t b = 1; b < c->S.N; ++b) c->blen[b] = new_branches[b];
  HIP_TRY(c, hipMemcpyAsync(c->d_blen, c->blen.data(), sizeof(double) * c->S.N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->have_reset = false;  // cached log-likelihoods are stale, as in the reference
  return EPV_OK;
}

static int export_paths(epv_ctx *c, uint8_t *init_state, uint64_t *offsets, double *jumps,
                        uint64_t *total) {
  const uint64_t E = (uint64_t)c->S.B * c->S.n;
  DevTmp<uint8_t> init_tmp;
  DevTmp<uint64_t> cnt_tmp;
  HIP_TRY(c, init_tmp.alloc(E));
  HIP_TRY(c, cnt_tmp.alloc(E + 1));
  uint8_t *d_init = init_tmp.p;
  uint64_t *d_cnt = cnt_tmp.p;
  hipLaunchKernelGGL(epv_count_kernel, dim3((unsigned)((E + 255u) / 256u)), dim3(256), 0, c->stream,
                     c->S, d_init, d_cnt);
  std::vector<uint64_t> off(E + 1);
  HIP_TRY(c, hipMemcpyAsync(off.data(), d_cnt, E * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  uint64_t run = 0;
  for (uint64_t e = 0; e < E; ++e) { const uint64_t k = off[e]; off[e] = run; run += k; }
  off[E] = run;
  if (total) *total = run;
  if (offsets) {
    std::memcpy(offsets, off.data(), (E + 1) * sizeof(uint64_t));
    HIP_TRY(c, hipMemcpy(init_state, d_init, E, hipMemcpyDeviceToHost));
    if (run) {
      DevTmp<double> j_tmp;
      HIP_TRY(c, j_tmp.alloc(run));
      double *d_j = j_tmp.p;
      HIP_TRY(c, hipMemcpyAsync(d_cnt, off.data(), (E + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
      hipLaunchKernelGGL(epv_gather_kernel, dim3((unsigned)((E + 255u) / 256u)), dim3(256), 0,
                         c->stream, c->S, d_cnt, d_j);
      HIP_TRY(c, hipMemcpyAsync(jumps, d_j, run * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
  }
  return EPV_OK;
}

EPV_API int epv_paths_total_jumps(epv_ctx *c, uint64_t *total) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  return export_paths(c, nullptr, nullptr, nullptr, total);
}

EPV_API int epv_download_paths(epv_ctx *c, uint8_t *init_state, uint64_t *offsets, double *jumps) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (!init_state || !offsets) return fail(c, EPV_ERR_ARG, "null output");
  HIP_TRY(c, hipSetDevice(c->device));
  return export_paths(c, init_state, offsets, jumps, nullptr);
}

EPV_API int epv_get_tri_llh(epv_ctx *c, double *out) {
  int rc = check_ready(c, true);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpy(out, c->S.tri, c->S.n * sizeof(double), hipMemcpyDeviceToHost));
  return EPV_OK;
}

EPV_API uint64_t epv_column_bytes(const epv_ctx *c) {
  if (!c || !c->have_paths) return 0;
  return (((uint64_t)c->S.B * sizeof(epv_meta_t) + 7u) & ~7ull) + ((uint64_t)c->S.B * c->S.C + 3u) * 8u;
}

EPV_API int epv_get_columns(epv_ctx *c, uint64_t first, uint64_t count, void *packed) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (first + count > c->S.n || !packed) return fail(c, EPV_ERR_ARG, "bad column range");
  if (count == 0) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t bytes = count * epv_column_bytes(c);
  if ((rc = ensure_stage(c, bytes))) return rc;
  uint8_t *d = c->d_stage;
  hipLaunchKernelGGL(epv_pack_columns_kernel, dim3((unsigned)count), dim3(64), 0, c->stream, c->S,
                     first, count, d);
  HIP_TRY(c, hipMemcpyAsync(packed, d, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}

// columns [src_first, src_first+count) of `src` -> columns [dst_first, ...) of `dst`, both on
// the same GPU, without leaving it (halo refresh between the shards of a LocalGroup)
EPV_API int epv_copy_columns(epv_ctx *src, uint64_t src_first, uint64_t count, epv_ctx *dst,
                             uint64_t dst_first) {
  int rc = check_ready(src, false);
  if (rc) return rc;
  if ((rc = check_ready(dst, false))) return rc;
  if (src->device != dst->device || src->S.B != dst->S.B || src->S.C != dst->S.C)
    return fail(dst, EPV_ERR_ARG, "epv_copy_columns needs two contexts of one GPU with equal tree and capacity");
  if (src_first + count > src->S.n || dst_first + count > dst->S.n) return fail(dst, EPV_ERR_ARG, "bad column range");
  if (count == 0) return EPV_OK;
  HIP_TRY(src, hipSetDevice(src->device));
  const uint64_t bytes = count * epv_column_bytes(src);
  if ((rc = ensure_stage(src, bytes))) return rc;
  hipLaunchKernelGGL(epv_pack_columns_kernel, dim3((unsigned)count), dim3(64), 0, src->stream, src->S,
                     src_first, count, src->d_stage);
  HIP_TRY(src, hipGetLastError());
  HIP_TRY(src, hipStreamSynchronize(src->stream));
  hipLaunchKernelGGL(epv_unpack_columns_kernel, dim3((unsigned)count), dim3(64), 0, dst->stream, dst->S,
                     dst_first, count, src->d_stage);
  HIP_TRY(dst, hipGetLastError());
  HIP_TRY(dst, hipStreamSynchronize(dst->stream));
  return EPV_OK;
}

// the same without a host synchronisation: the columns are packed on src's stream into half `slot`
// (0 or 1) of its staging buffer and unpacked on dst's stream behind an event -- whatever the caller
// launches on dst's stream afterwards (epv_reset) sees them; src must not be asked for the same slot
// again before dst's stream has passed the unpack
EPV_API int epv_copy_columns_async(epv_ctx *src, uint64_t src_first, uint64_t count, epv_ctx *dst,
                                   uint64_t dst_first, int slot) {
  int rc = check_ready(src, false);
  if (rc) return rc;
  if ((rc = check_ready(dst, false))) return rc;
  if (slot < 0 || slot > 1) return fail(dst, EPV_ERR_ARG, "slot must be 0 or 1");
  if (src->device != dst->device || src->S.B != dst->S.B || src->S.C != dst->S.C)
    return fail(dst, EPV_ERR_ARG, "epv_copy_columns_async needs two contexts of one GPU with equal tree and capacity");
  if (src_first + count > src->S.n || dst_first + count > dst->S.n) return fail(dst, EPV_ERR_ARG, "bad column range");
  if (count == 0) return EPV_OK;
  HIP_TRY(src, hipSetDevice(src->device));
  const uint64_t bytes = count * epv_column_bytes(src);
  if (2u * bytes > src->stage_cap) {
    // (growing the buffer waits for both streams: a half of it may still be read)
    HIP_TRY(dst, hipStreamSynchronize(dst->stream));
    if ((rc = ensure_stage(src, 2u * bytes))) return rc;
  }
  if (!src->ev_copy[slot]) HIP_TRY(src, hipEventCreateWithFlags(&src->ev_copy[slot], hipEventDisableTiming));
  uint8_t *stage = src->d_stage + (slot ? src->stage_cap / 2u : 0u);
  hipLaunchKernelGGL(epv_pack_columns_kernel, dim3((unsigned)count), dim3(64), 0, src->stream, src->S,
                     src_first, count, stage);
  HIP_TRY(src, hipGetLastError());
  HIP_TRY(src, hipEventRecord(src->ev_copy[slot], src->stream));
  HIP_TRY(dst, hipStreamWaitEvent(dst->stream, src->ev_copy[slot], 0));
  hipLaunchKernelGGL(epv_unpack_columns_kernel, dim3((unsigned)count), dim3(64), 0, dst->stream, dst->S,
                     dst_first, count, stage);
  HIP_TRY(dst, hipGetLastError());
  return EPV_OK;
}

// the same with the packed columns staying in DEVICE memory of the context's GPU (a buffer the
// caller hands to RCCL): nothing passes through the host
EPV_API int epv_pack_columns_dev(epv_ctx *c, uint64_t first, uint64_t count, void *d_packed) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (first + count > c->S.n || !d_packed) return fail(c, EPV_ERR_ARG, "bad column range");
  if (count == 0) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(epv_pack_columns_kernel, dim3((unsigned)count), dim3(64), 0, c->stream, c->S,
                     first, count, static_cast<uint8_t *>(d_packed));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}
EPV_API int epv_unpack_columns_dev(epv_ctx *c, uint64_t first, uint64_t count, const void *d_packed) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (first + count > c->S.n || !d_packed) return fail(c, EPV_ERR_ARG, "bad column range");
  if (count == 0) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(epv_unpack_columns_kernel, dim3((unsigned)count), dim3(64), 0, c->stream, c->S,
                     first, count, static_cast<const uint8_t *>(d_packed));
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}
EPV_API int epv_device_of(const epv_ctx *c) { return c ? c->device : -1; }

EPV_API int epv_put_columns(epv_ctx *c, uint64_t first, uint64_t count, const void *packed) {
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (first + count > c->S.n || !packed) return fail(c, EPV_ERR_ARG, "bad column range");
  if (count == 0) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint64_t bytes = count * epv_column_bytes(c);
  if ((rc = ensure_stage(c, bytes))) return rc;
  uint8_t *d = c->d_stage;
  HIP_TRY(c, hipMemcpyAsync(d, packed, bytes, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(epv_unpack_columns_kernel, dim3((unsigned)count), dim3(64), 0, c->stream, c->S,
                     first, count, d);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}

EPV_API int epv_get_counters(epv_ctx *c, epv_counters *out) {
  if (!c || !out) return EPV_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long cnt[EPV_CNT_N];
  int rc = read_counters(c, cnt);
  if (rc) return rc;
  out->n_overflow = cnt[EPV_CNT_OVERFLOW];
  out->n_coop_tasks = cnt[EPV_CNT_COOP];
  out->n_sweeps = c->n_sweeps;
  out->n_search_finished = cnt[EPV_CNT_SEARCH_FINISHED];
  return EPV_OK;
}

#ifdef EPV_P2_PROFILE
// sums over the per-wave rows: out[0..14] section cycles, out[15] waves
EPV_API int epv_debug_p2_profile(unsigned long long *out) {
  std::vector<unsigned long long> rows(16u * EPV_P2_PROF_ROWS);
  if (hipMemcpyFromSymbol(rows.data(), HIP_SYMBOL(epv_p2_prof), rows.size() * sizeof(unsigned long long)) != hipSuccess) return 1;
  for (int q = 0; q < 16; ++q) out[q] = 0;
  for (size_t r = 0; r < EPV_P2_PROF_ROWS; ++r)
    for (int q = 0; q < 16; ++q) out[q] += rows[16u * r + q];
  return 0;
}
// what hipOccupancyMaxActiveBlocksPerMultiprocessor says for the fused kernel this context would launch, at the
// launch's dynamic LDS: blocks (one wave each) per CU
EPV_API int epv_debug_p2_occupancy(epv_ctx *c, int *blocks, unsigned long long *lds) {
  if (!c || !blocks || !lds || !c->have_paths) return EPV_ERR_ARG;
  const PhasePlan P = phase_plan(c);
  if (P.propose != EPV_PLAN_FUSED) return EPV_ERR_STATE;
  *lds = c->shapes.v2.lds;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void *>(fused_kernel(P.small_nn, P.direct)), 64,
                                                      c->shapes.v2.lds) == hipSuccess ? EPV_OK : EPV_ERR_HIP;
}
#endif

EPV_API int epv_set_timing(epv_ctx *c, int enabled) {
  if (!c) return EPV_ERR_ARG;
  c->timing_every = enabled > 0 ? (uint32_t)enabled : 0u;
  c->timing_seen = 0;
  c->timing = false;
  return EPV_OK;
}

EPV_API int epv_kernel_time_ms(epv_ctx *c, double *avg_ms, uint64_t *n_launches) {
  if (!c || !avg_ms || !n_launches) return EPV_ERR_ARG;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  int rc = drain_timing(c);
  if (rc) return rc;
  *n_launches = c->timed_launches;
  *avg_ms = c->timed_launches ? c->timed_ms / (double)c->timed_launches : 0.0;
  c->timed_ms = 0.0;
  c->timed_launches = 0;
  return EPV_OK;
}

// ---- average history of the sampled paths (epv_pavg.h)
EPV_API int epv_set_path_average(epv_ctx *c, uint32_t n_points) {
  if (n_points == 0) return layer_set_off(c, kPavg);
  int rc = check_ready(c, false);
  if (rc) return rc;
  if (n_points < 2) return fail(c, EPV_ERR_ARG, "a path average needs at least 2 points");
  HIP_TRY(c, hipSetDevice(c->device));
  c->pa.P = n_points;
  if ((rc = relayout(c, kPavg, pavg_alloc)) || (rc = ensure_pavg(c))) return rc;   // (the grid as well)
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}

EPV_API int epv_reset_path_average(epv_ctx *c) {
  const int rc = layer_entry(c, kPavg);
  if (rc) return rc;
  if (c->pa.d)
    HIP_TRY(c, hipMemsetAsync(c->pa.d, 0, (size_t)4u * c->pa.at.B * c->pa.at.cnt * c->pa.P, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->pa.samples = 0;
  return EPV_OK;
}

EPV_API int epv_accumulate_path_average(epv_ctx *c) { return layer_accumulate(c, kPavg); }

EPV_API int epv_path_average_samples(epv_ctx *c, uint64_t *n) {
  if (!c || !n) return EPV_ERR_ARG;
  *n = c->pa.samples;   // (0 while the layer is off)
  return EPV_OK;
}

EPV_API int epv_path_average_layout(epv_ctx *c, uint32_t *n_points, uint64_t *first, uint64_t *count) {
  if (!c || !n_points || !first || !count) return EPV_ERR_ARG;
  *n_points = 0;
  *first = *count = 0;
  if (!c->pa.P) return EPV_OK;
  if (c->have_tree && c->have_paths) {   // (no samples yet: lay out for the sites as they are now)
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_pavg(c);
    if (rc && c->pa.samples == 0) return rc;
  }
  *n_points = c->pa.P;
  *first = c->pa.at.lo;
  *count = c->pa.at.cnt;
  return EPV_OK;
}

EPV_API int epv_get_path_average(epv_ctx *c, uint64_t first, uint64_t count, uint32_t *counts) {
  int rc = layer_entry(c, kPavg);
  if (rc) return rc;
  if (!counts) return fail(c, EPV_ERR_ARG, "null output");
  if (first < c->pa.at.lo || first + count > c->pa.at.lo + c->pa.at.cnt)
    return fail(c, EPV_ERR_ARG, "site range outside the sites this context averages");
  if (count == 0) return EPV_OK;
  const uint64_t bytes = (uint64_t)4u * c->pa.at.B * count * c->pa.P;
  if ((rc = grow_staging(c, &c->pa.d_out, &c->pa.out_cap, bytes))) return rc;
  hipLaunchKernelGGL(epv_pavg_read_kernel, dim3((unsigned)((count + EPV_PAVG_RD - 1u) / EPV_PAVG_RD), c->pa.at.B),
                     dim3(EPV_PAVG_RD), 0, c->stream, (const int32_t *)c->pa.d, c->pa.P, c->pa.at.cnt,
                     first - c->pa.at.lo, count, c->pa.d_out);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(counts, c->pa.d_out, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}

// ---- posterior branch-event maps (epv_bevents.h)
EPV_API int epv_set_branch_events(epv_ctx *c, int on) {
  if (!on) return layer_set_off(c, kBevents);
  const int rc = check_ready(c, false);
  if (rc) return rc;
  c->be.on = true;
  return layer_set_on(c, kBevents, bevents_alloc);
}

EPV_API int epv_reset_branch_events(epv_ctx *c) {
  const int rc = layer_entry(c, kBevents);
  if (rc) return rc;
  if (c->be.d)
    HIP_TRY(c, hipMemsetAsync(c->be.d, 0, (size_t)4u * EPV_BEV_PLANES * c->be.at.B * c->be.at.cnt, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->be.samples = 0;
  return EPV_OK;
}

EPV_API int epv_accumulate_branch_events(epv_ctx *c) { return layer_accumulate(c, kBevents); }

EPV_API int epv_branch_events_samples(epv_ctx *c, uint64_t *n) {
  if (!c || !n) return EPV_ERR_ARG;
  *n = c->be.samples;   // (0 while the layer is off)
  return EPV_OK;
}

EPV_API int epv_branch_events_set_samples(epv_ctx *c, uint64_t n) {
  const int rc = layer_entry(c, kBevents);
  if (rc) return rc;
  c->be.samples = n;
  return EPV_OK;
}

EPV_API int epv_branch_events_layout(epv_ctx *c, uint64_t *first, uint64_t *count) {
  if (!c || !first || !count) return EPV_ERR_ARG;
  *first = *count = 0;
  if (!c->be.on) return EPV_OK;
  if (c->have_tree && c->have_paths) {   // (no samples yet: lay out for the sites as they are now)
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_bevents(c);
    if (rc && c->be.samples == 0) return rc;
  }
  *first = c->be.at.lo;
  *count = c->be.at.cnt;
  return EPV_OK;
}

EPV_API int epv_get_branch_events(epv_ctx *c, uint64_t first, uint64_t count, uint32_t *planes) {
  const int rc = layer_entry(c, kBevents);
  if (rc) return rc;
  if (!planes) return fail(c, EPV_ERR_ARG, "null output");
  if (first < c->be.at.lo || first + count > c->be.at.lo + c->be.at.cnt)
    return fail(c, EPV_ERR_ARG, "site range outside the sites this context counts");
  if (count == 0) return EPV_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // rows of `count` sites out of rows of at.cnt: [6 B][at.cnt] -> [6 B][count]
  HIP_TRY(c, hipMemcpy2D(planes, count * 4u, c->be.d + (first - c->be.at.lo), c->be.at.cnt * 4u, count * 4u,
                         (size_t)EPV_BEV_PLANES * c->be.at.B, hipMemcpyDeviceToHost));
  return EPV_OK;
}

EPV_API int epv_get_branch_event_windows(epv_ctx *c, uint64_t W, uint64_t first_window, uint64_t n_windows,
                                         uint64_t *sums) {
  const int rc = layer_entry(c, kBevents);
  if (rc) return rc;
  return row_window_sums(c, c->be.d, (uint64_t)EPV_BEV_PLANES * c->be.at.B, c->be.at, &c->be.d_out, &c->be.out_cap, W,
                         first_window, n_windows, sums);
}

// ---- chain mixing diagnostics (epv_mixing.h)
EPV_API int epv_set_mixing(epv_ctx *c, uint32_t max_lag) {
  if (!max_lag) return layer_set_off(c, kMixing);
  const int rc = check_ready(c, false);
  if (rc) return rc;
  if (max_lag > EPV_MIX_MAX_LAG) return fail(c, EPV_ERR_ARG, "max_lag of the mixing diagnostics: 1 .. 16 (0 turns them off)");
  c->mx.K = max_lag;
  return layer_set_on(c, kMixing, mixing_alloc);
}

EPV_API int epv_reset_mixing(epv_ctx *c) {
  int rc = layer_entry(c, kMixing);
  if (rc) return rc;
  if ((rc = mixing_zero(c))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}

EPV_API int epv_accumulate_mixing(epv_ctx *c) { return layer_accumulate(c, kMixing); }

EPV_API int epv_mixing_samples(epv_ctx *c, uint64_t *n) {
  if (!c || !n) return EPV_ERR_ARG;
  *n = c->mx.samples;   // (0 while the layer is off)
  return EPV_OK;
}

EPV_API int epv_mixing_layout(epv_ctx *c, uint64_t *first, uint64_t *count, uint32_t *max_lag) {
  if (!c || !first || !count || !max_lag) return EPV_ERR_ARG;
  *first = *count = 0;
  *max_lag = 0;
  if (!c->mx.K) return EPV_OK;
  if (c->have_tree && c->have_paths) {   // (no samples yet: lay out for the sites as they are now)
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_mixing(c);
    if (rc && c->mx.samples == 0) return rc;
  }
  *first = c->mx.at.lo;
  *count = c->mx.at.cnt;
  *max_lag = c->mx.K;
  return EPV_OK;
}

EPV_API int epv_mixing_pairs(epv_ctx *c, uint64_t *words) {
  const int rc = layer_entry(c, kMixing);
  if (rc) return rc;
  if (!words) return fail(c, EPV_ERR_ARG, "null output");
  words[0] = c->mx.samples;
  words[1] = c->mx.moved_pairs;
  for (uint32_t k = 1; k <= c->mx.K; ++k) words[1u + k] = c->mx.pairs[k];
  return EPV_OK;
}

EPV_API int epv_mixing_counts(epv_ctx *c, uint64_t first, uint64_t count, uint32_t *moved, uint64_t *sums) {
  const int rc = layer_entry(c, kMixing);
  if (rc) return rc;
  if (!moved || !sums) return fail(c, EPV_ERR_ARG, "null output");
  if (first < c->mx.at.lo || first + count > c->mx.at.lo + c->mx.at.cnt)
    return fail(c, EPV_ERR_ARG, "site range outside the sites this context counts");
  if (count == 0) return EPV_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint64_t off = first - c->mx.at.lo;
  HIP_TRY(c, hipMemcpy(moved, c->mx.d_moved + off, count * 4u, hipMemcpyDeviceToHost));
  // rows of `count` sites out of rows of at.cnt: [2 + K][at.cnt] -> [2 + K][count]
  HIP_TRY(c, hipMemcpy2D(sums, count * 8u, c->mx.d_sums + off, c->mx.at.cnt * 8u, count * 8u, 2u + c->mx.K,
                         hipMemcpyDeviceToHost));
  return EPV_OK;
}

EPV_API int epv_mixing_windows(epv_ctx *c, uint64_t W, uint64_t first_window, uint64_t n_windows, uint64_t *sums) {
  const int rc = layer_entry(c, kMixing);
  if (rc) return rc;
  return row_window_sums(c, c->mx.d_moved, 1u, c->mx.at, &c->mx.d_out, &c->mx.out_cap, W, first_window, n_windows, sums);
}

// ---- change patterns (epv_patterns.h)
EPV_API int epv_set_change_patterns(epv_ctx *c, int on) {
  if (!on) return layer_set_off(c, kPatterns);
  const int rc = check_ready(c, false);
  if (rc) return rc;
  c->pt.on = true;
  return layer_set_on(c, kPatterns, patterns_alloc);
}

EPV_API int epv_reset_change_patterns(epv_ctx *c) {
  const int rc = layer_entry(c, kPatterns);
  if (rc) return rc;
  if (c->pt.d) HIP_TRY(c, hipMemsetAsync(c->pt.d, 0, (size_t)4u * c->pt.R * c->pt.at.cnt, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->pt.samples = 0;
  return EPV_OK;
}

EPV_API int epv_accumulate_change_patterns(epv_ctx *c) { return layer_accumulate(c, kPatterns); }

EPV_API int epv_change_patterns_samples(epv_ctx *c, uint64_t *n) {
  if (!c || !n) return EPV_ERR_ARG;
  *n = c->pt.samples;   // (0 while the layer is off)
  return EPV_OK;
}

EPV_API int epv_change_patterns_layout(epv_ctx *c, uint32_t *n_rows, uint32_t *n_clades, uint32_t *clade_node,
                                       uint64_t *first, uint64_t *count) {
  if (!c || !n_rows || !n_clades || !first || !count) return EPV_ERR_ARG;
  *n_rows = *n_clades = 0;
  *first = *count = 0;
  if (!c->pt.on) return EPV_OK;
  if (c->have_tree && c->have_paths) {   // (no samples yet: lay out for the tree and sites as they are now)
    HIP_TRY(c, hipSetDevice(c->device));
    int rc = ensure_patterns(c);
    if (rc && c->pt.samples == 0) return rc;
  }
  *n_rows = c->pt.R;
  *n_clades = c->pt.I;
  *first = c->pt.at.lo;
  *count = c->pt.at.cnt;
  if (clade_node)
    for (uint32_t v = 1, j = 0; v < c->pt.subtree.size(); ++v)
      if (c->pt.subtree[v] > 1u) clade_node[j++] = v;
  return EPV_OK;
}

EPV_API int epv_get_change_patterns(epv_ctx *c, uint64_t first, uint64_t count, uint32_t *rows) {
  const int rc = layer_entry(c, kPatterns);
  if (rc) return rc;
  if (!rows) return fail(c, EPV_ERR_ARG, "null output");
  if (first < c->pt.at.lo || first + count > c->pt.at.lo + c->pt.at.cnt)
    return fail(c, EPV_ERR_ARG, "site range outside the sites this context counts");
  if (count == 0) return EPV_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // rows of `count` sites out of rows of at.cnt: [R][at.cnt] -> [R][count]
  HIP_TRY(c, hipMemcpy2D(rows, count * 4u, c->pt.d + (first - c->pt.at.lo), c->pt.at.cnt * 4u, count * 4u, c->pt.R,
                         hipMemcpyDeviceToHost));
  return EPV_OK;
}

EPV_API int epv_get_change_pattern_windows(epv_ctx *c, uint64_t W, uint64_t first_window, uint64_t n_windows,
                                           uint64_t *sums) {
  const int rc = layer_entry(c, kPatterns);
  if (rc) return rc;
  return row_window_sums(c, c->pt.d, c->pt.R, c->pt.at, &c->pt.d_out, &c->pt.out_cap, W, first_window, n_windows, sums);
}

// ---- regional sufficient statistics (epv_wstat.h)
EPV_API int epv_set_window_stats(epv_ctx *c, uint64_t W) {
  if (!W) return layer_set_off(c, kWstat);
  if (const int frc = refuse_fixed(c, kWstat)) return frc;
  const int rc = check_ready(c, false);
  if (rc) return rc;
  c->ws.W_asked = W;
  return layer_set_on(c, kWstat, wstat_alloc);
}

EPV_API int epv_reset_window_stats(epv_ctx *c) {
  const int rc = layer_entry(c, kWstat);
  if (rc) return rc;
  if (c->ws.d) HIP_TRY(c, hipMemsetAsync(c->ws.d, 0, (size_t)128u * c->ws.at.B * c->ws.nw, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->ws.samples = 0;
  c->ws.scale.clear();
  return EPV_OK;
}

EPV_API int epv_accumulate_window_stats(epv_ctx *c) { return layer_accumulate(c, kWstat); }

EPV_API int epv_window_stats_samples(epv_ctx *c, uint64_t *n) {
  if (!c || !n) return EPV_ERR_ARG;
  *n = c->ws.samples;   // (0 while the layer is off)
  return EPV_OK;
}

EPV_API int epv_window_stats_set_samples(epv_ctx *c, uint64_t n) {
  int rc = layer_entry(c, kWstat);
  if (rc) return rc;
  if (n && c->ws.scale.empty()) {   // (as if the samples had been taken with the scales of now)
    if ((rc = ensure_stat_scale(c))) return rc;
    c->ws.scale = c->statscale;
  }
  c->ws.samples = n;
  if (!n) c->ws.scale.clear();
  return EPV_OK;
}

EPV_API int epv_window_stats_scale_exps(epv_ctx *c, int *k) {
  if (!k) return EPV_ERR_ARG;
  int rc = layer_entry(c, kWstat);
  if (rc) return rc;
  if (!c->have_tree) return fail(c, EPV_ERR_STATE, "epv_set_tree must come first");
  if (c->ws.scale.empty() && (rc = ensure_stat_scale(c))) return rc;
  const std::vector<double> &sc = c->ws.scale.empty() ? c->statscale : c->ws.scale;
  for (uint32_t b = 1; b < c->S.N && b < sc.size(); ++b) k[b - 1u] = std::ilogb(sc[b]);   // (sc[b] = 2^k_b exactly)
  return EPV_OK;
}

EPV_API int epv_window_stats_layout(epv_ctx *c, uint64_t *W, uint64_t *first_window, uint64_t *n_windows) {
  if (!c || !W || !first_window || !n_windows) return EPV_ERR_ARG;
  *W = *first_window = *n_windows = 0;
  if (!c->ws.W) return EPV_OK;
  if (c->have_tree && c->have_paths && c->ws.samples == 0) {   // lay out for the sites as they are now
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = ensure_wstat(c);
    if (rc) return rc;
  }
  *W = c->ws.W;
  *first_window = c->ws.w0;
  *n_windows = c->ws.nw;
  return EPV_OK;
}

EPV_API int epv_get_window_stats(epv_ctx *c, uint64_t first_window, uint64_t n_windows, int64_t *counts) {
  const int rc = layer_entry(c, kWstat);
  if (rc) return rc;
  if (!counts) return fail(c, EPV_ERR_ARG, "null output");
  if (first_window + n_windows < first_window) return fail(c, EPV_ERR_ARG, "window range overflows");
  if (n_windows == 0) return EPV_OK;
  const uint64_t V = (uint64_t)c->ws.at.B * 16u;
  std::memset(counts, 0, n_windows * V * sizeof(int64_t));
  const uint64_t a = std::max(first_window, c->ws.w0), e = std::min(first_window + n_windows, c->ws.w0 + c->ws.nw);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (a < e)
    HIP_TRY(c, hipMemcpy(counts + (a - first_window) * V, c->ws.d + (a - c->ws.w0) * V, (e - a) * V * sizeof(int64_t),
                         hipMemcpyDeviceToHost));
  return EPV_OK;
}

// ---- lineage origin maps (epv_origin.h)
EPV_API int epv_set_lineage_origins(epv_ctx *c, int on) {
  if (!on) return layer_set_off(c, kOrigins);
  const int rc = check_ready(c, false);
  if (rc) return rc;
  c->lo.on = true;
  return layer_set_on(c, kOrigins, origins_alloc);
}

EPV_API int epv_reset_lineage_origins(epv_ctx *c) {
  const int rc = layer_entry(c, kOrigins);
  if (rc) return rc;
  if (c->lo.d) HIP_TRY(c, hipMemsetAsync(c->lo.d, 0, (size_t)4u * c->lo.R * c->lo.at.cnt, c->stream));
  if (c->lo.d_age) HIP_TRY(c, hipMemsetAsync(c->lo.d_age, 0, (size_t)8u * c->lo.L * c->lo.at.cnt, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->lo.samples = 0;
  return EPV_OK;
}

EPV_API int epv_accumulate_lineage_origins(epv_ctx *c) { return layer_accumulate(c, kOrigins); }

EPV_API int epv_lineage_origins_samples(epv_ctx *c, uint64_t *n) {
  if (!c || !n) return EPV_ERR_ARG;
  *n = c->lo.samples;   // (0 while the layer is off)
  return EPV_OK;
}

EPV_API int epv_lineage_origins_set_samples(epv_ctx *c, uint64_t n) {
  const int rc = layer_entry(c, kOrigins);
  if (rc) return rc;
  c->lo.samples = n;
  return EPV_OK;
}

// (no samples yet: lay out for the tree and the sites as they are now)
static int origins_current(epv_ctx *c) {
  if (!c->have_tree || !c->have_paths || c->lo.samples) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return ensure_origins(c);
}

EPV_API int epv_lineage_origins_layout(epv_ctx *c, uint32_t *n_leaves, uint32_t *n_rows, uint64_t *first,
                                       uint64_t *count) {
  if (!c || !n_leaves || !n_rows || !first || !count) return EPV_ERR_ARG;
  *n_leaves = *n_rows = 0;
  *first = *count = 0;
  if (!c->lo.on) return EPV_OK;
  const int rc = origins_current(c);
  if (rc) return rc;
  *n_leaves = c->lo.L;
  *n_rows = c->lo.R;
  *first = c->lo.at.lo;
  *count = c->lo.at.cnt;
  return EPV_OK;
}

EPV_API int epv_lineage_origin_rows(epv_ctx *c, uint32_t *leaf_node, uint32_t *branch_node) {
  if (!leaf_node || !branch_node) return EPV_ERR_ARG;
  int rc = layer_entry(c, kOrigins);
  if (rc || (rc = origins_current(c))) return rc;
  std::copy(c->lo.leaf.begin(), c->lo.leaf.end(), leaf_node);
  std::copy(c->lo.rowb.begin(), c->lo.rowb.end(), branch_node);
  return EPV_OK;
}

EPV_API int epv_lineage_origins_scale_exp(epv_ctx *c, int *k) {
  if (!k) return EPV_ERR_ARG;
  int rc = layer_entry(c, kOrigins);
  if (rc || (rc = origins_current(c))) return rc;
  *k = c->lo.k;
  return EPV_OK;
}

EPV_API int epv_get_lineage_origins(epv_ctx *c, uint64_t first, uint64_t count, uint32_t *origin, uint64_t *age) {
  const int rc = layer_entry(c, kOrigins);
  if (rc) return rc;
  if (!origin || !age) return fail(c, EPV_ERR_ARG, "null output");
  if (first < c->lo.at.lo || first + count > c->lo.at.lo + c->lo.at.cnt)
    return fail(c, EPV_ERR_ARG, "site range outside the sites this context counts");
  if (count == 0) return EPV_OK;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // rows of `count` sites out of rows of at.cnt
  HIP_TRY(c, hipMemcpy2D(origin, count * 4u, c->lo.d + (first - c->lo.at.lo), c->lo.at.cnt * 4u, count * 4u, c->lo.R,
                         hipMemcpyDeviceToHost));
  HIP_TRY(c, hipMemcpy2D(age, count * 8u, c->lo.d_age + (first - c->lo.at.lo), c->lo.at.cnt * 8u, count * 8u, c->lo.L,
                         hipMemcpyDeviceToHost));
  return EPV_OK;
}

EPV_API int epv_get_lineage_origin_windows(epv_ctx *c, uint64_t W, uint64_t first_window, uint64_t n_windows,
                                           uint64_t *out) {
  int rc = layer_entry(c, kOrigins);
  if (rc) return rc;
  if (!out) return fail(c, EPV_ERR_ARG, "null output");
  if (W == 0) return fail(c, EPV_ERR_ARG, "a window holds at least one site");
  if (first_window + n_windows < first_window) return fail(c, EPV_ERR_ARG, "window range overflows");
  if (n_windows == 0) return EPV_OK;
  const uint64_t rows = c->lo.R, bytes = rows * n_windows * 8u;
  std::memset(out, 0, ((uint64_t)c->lo.R + c->lo.L) * n_windows * 8u);
  if (c->lo.at.cnt == 0 || c->lo.at.ng == 0 || rows == 0) return EPV_OK;   // this context counts no site
  if ((rc = grow_staging(c, &c->lo.d_out, &c->lo.out_cap, bytes))) return rc;
  if (W > c->lo.at.ng) W = c->lo.at.ng;   // one window holds the genome: the same sums, and w W cannot overflow
  uint32_t Wp = 256u;
  if (W <= 64u) for (Wp = 1u; Wp < W; Wp <<= 1) {}
  const uint64_t per_block = 256u / Wp, blocks = (n_windows + per_block - 1u) / per_block;
  if (blocks > 0x7fffffffull) return fail(c, EPV_ERR_ARG, "too many windows in one call: read them out in pieces");
  // (the branch events' window kernel: generic uint32 rows x cnt, blockIdx.y = row; a deep tree has more rows
  // than a grid's y dimension takes)
  for (uint64_t r0 = 0; r0 < rows; r0 += 65535u) {
    const uint64_t nr = std::min<uint64_t>(65535u, rows - r0);
    hipLaunchKernelGGL(epv_bevents_window_kernel, dim3((unsigned)blocks, (unsigned)nr), dim3(256), 0, c->stream,
                       (const uint32_t *)c->lo.d + r0 * c->lo.at.cnt, c->lo.R, c->lo.at.cnt, c->lo.at.g0 + c->lo.at.lo, c->lo.at.ng, W,
                       Wp, first_window, n_windows, c->lo.d_out + r0 * n_windows);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipMemcpyAsync(out, c->lo.d_out, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  // the ages are 64-bit cells, which the window kernel does not take: the counted sites that lie in the asked
  // windows come to the host and are added there, in 128 bits so that a sum beyond 64 is refused, not wrapped
  const uint64_t glo = c->lo.at.g0 + c->lo.at.lo, n_win = (c->lo.at.ng + W - 1u) / W;
  const uint64_t w_end = std::min(first_window + n_windows, n_win);
  if (first_window >= w_end) return EPV_OK;
  const uint64_t a = std::max(first_window * W, glo), e = std::min(std::min(w_end * W, c->lo.at.ng), glo + c->lo.at.cnt);
  if (a >= e) return EPV_OK;
  // in pieces of sites (512 KB of cells on the host at a time, or 1024 sites of every leaf); a window that
  // straddles two pieces gets both parts
  const uint64_t piece = std::max<uint64_t>(1024u, (1ull << 16) / c->lo.L);
  try {
    std::vector<unsigned long long> cells((size_t)c->lo.L * std::min(piece, e - a));
    for (uint64_t p0 = a; p0 < e; p0 += piece) {
      const uint64_t p1 = std::min(p0 + piece, e), len = p1 - p0;
      HIP_TRY(c, hipMemcpy2D(cells.data(), len * 8u, c->lo.d_age + (p0 - glo), c->lo.at.cnt * 8u, len * 8u, c->lo.L,
                             hipMemcpyDeviceToHost));
      for (uint32_t l = 0; l < c->lo.L; ++l) {
        const unsigned long long *p = cells.data() + (size_t)l * len;
        uint64_t *o = out + (rows + l) * n_windows;
        for (uint64_t g = p0; g < p1;) {
          const uint64_t w = g / W, stop = std::min((w + 1u) * W, p1);
          unsigned __int128 sum = o[w - first_window];
          for (; g < stop; ++g) sum += p[g - p0];
          if (sum >> 64)
            return fail(c, EPV_ERR_ARG, "the age sum of a window passes 64 bits: use narrower windows");
          o[w - first_window] = (uint64_t)sum;
        }
      }
    }
  } catch (const std::bad_alloc &) {
    return fail(c, EPV_ERR_ARG, "no host memory for a piece of the lineage origins' ages");
  }
  return EPV_OK;
}

// ---- the entry points of the summaries that are joint along the genome
// what epv_*_layout begins with while the layer is on: no samples yet, so lay out for the tree and sites as they are now
static int part_layout_entry(epv_ctx *c, const PartKind &K, const PartState &p) {
  if (!c->have_tree || !c->have_paths || p.samples) return EPV_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return K.layer.ensure(c);
}
// epv_*_samples (0 while the layer is off)
static int part_samples(const epv_ctx *c, const PartState *p, uint64_t *n) {
  if (!c || !n) return EPV_ERR_ARG;
  *n = p->samples;
  return EPV_OK;
}
// epv_reset_*
static int part_reset(epv_ctx *c, const PartKind &K, PartState &p) {
  int rc = layer_entry(c, K.layer);
  if (rc || (rc = part_zero(c, p))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return EPV_OK;
}
// epv_get_*: the accumulators whole, the edge records of the samples held
static int part_get(epv_ctx *c, const PartKind &K, const PartState &p, void *acc0, void *acc1, uint64_t *edges) {
  const int rc = layer_entry(c, K.layer);
  if (rc) return rc;
  void *const acc[2] = {acc0, acc1};
  if (!edges || !acc0 || (p.shape.acc_b[1] && !acc1)) return fail(c, EPV_ERR_ARG, "null output");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int i = 0; i < 2; ++i)
    if (p.shape.acc_b[i]) HIP_TRY(c, hipMemcpy(acc[i], p.d_acc[i], p.shape.acc_b[i], hipMemcpyDeviceToHost));
  if (p.shape.edge_b * p.samples) HIP_TRY(c, hipMemcpy(edges, p.d_edge, p.shape.edge_b * p.samples, hipMemcpyDeviceToHost));
  return EPV_OK;
}


// ---- domain size spectra (epv_domains.h)
EPV_API int epv_set_domain_stats(epv_ctx *c, uint64_t max_samples) {
  if (!max_samples) return layer_set_off(c, kDomains);
  if (const int frc = refuse_fixed(c, kDomains)) return frc;
  if (max_samples > EPV_DOM_MAX_SAMPLES) return fail(c, EPV_ERR_ARG, "domain statistics take at most 2^21 samples");
  const int rc = check_ready(c, false);
  if (rc) return rc;
  c->dm.on = true;
  c->dm.max = max_samples;
  return layer_set_on(c, kDomains, domains_alloc);
}

EPV_API int epv_reset_domain_stats(epv_ctx *c) { return c ? part_reset(c, kDomainsPart, c->dm) : EPV_ERR_ARG; }

EPV_API int epv_accumulate_domain_stats(epv_ctx *c) { return layer_accumulate(c, kDomains); }

EPV_API int epv_domain_stats_samples(epv_ctx *c, uint64_t *n) { return part_samples(c, c ? &c->dm : nullptr, n); }

EPV_API int epv_domain_stats_layout(epv_ctx *c, uint32_t *n_nodes, uint32_t *n_bins, uint64_t *first, uint64_t *count,
                                    uint64_t *chunk_sites) {
  if (!c || !n_nodes || !n_bins || !first || !count || !chunk_sites) return EPV_ERR_ARG;
  *n_nodes = *n_bins = 0;
  *first = *count = *chunk_sites = 0;
  if (!c->dm.on) return EPV_OK;
  const int rc = part_layout_entry(c, kDomainsPart, c->dm);
  if (rc) return rc;
  *n_nodes = c->dm.shape.rows;
  *n_bins = EPV_DOM_BINS;
  *first = c->dm.at.lo;
  *count = c->dm.at.cnt;
  *chunk_sites = 64ull * EPV_DOM_CHUNK_WORDS;
  return EPV_OK;
}

EPV_API int epv_get_domain_stats(epv_ctx *c, uint64_t *hist, uint64_t *len_sum, uint64_t *edges) {
  return c ? part_get(c, kDomainsPart, c->dm, hist, len_sum, edges) : EPV_ERR_ARG;
}

// ---- domain turnover (epv_turnover.h)
EPV_API int epv_set_domain_turnover(epv_ctx *c, uint64_t max_samples) {
  if (!max_samples) return layer_set_off(c, kTurnover);
  if (const int frc = refuse_fixed(c, kTurnover)) return frc;
  if (max_samples > EPV_TURN_MAX_SAMPLES) return fail(c, EPV_ERR_ARG, "domain turnover takes at most 2^21 samples");
  const int rc = check_ready(c, false);
  if (rc) return rc;
  c->to.on = true;
  c->to.max = max_samples;
  return layer_set_on(c, kTurnover, turnover_alloc);
}

EPV_API int epv_reset_domain_turnover(epv_ctx *c) { return c ? part_reset(c, kTurnoverPart, c->to) : EPV_ERR_ARG; }

EPV_API int epv_accumulate_domain_turnover(epv_ctx *c) { return layer_accumulate(c, kTurnover); }

EPV_API int epv_domain_turnover_samples(epv_ctx *c, uint64_t *n) { return part_samples(c, c ? &c->to : nullptr, n); }

EPV_API int epv_domain_turnover_layout(epv_ctx *c, uint32_t *n_rows, uint32_t *n_bins, uint64_t *first, uint64_t *count,
                                       uint64_t *chunk_sites) {
  if (!c || !n_rows || !n_bins || !first || !count || !chunk_sites) return EPV_ERR_ARG;
  *n_rows = *n_bins = 0;
  *first = *count = *chunk_sites = 0;
  if (!c->to.on) return EPV_OK;
  const int rc = part_layout_entry(c, kTurnoverPart, c->to);
  if (rc) return rc;
  *n_rows = c->to.shape.rows;
  *n_bins = EPV_DOM_BINS;
  *first = c->to.at.lo;
  *count = c->to.at.cnt;
  *chunk_sites = 64ull * EPV_DOM_CHUNK_WORDS;
  return EPV_OK;
}

EPV_API int epv_get_domain_turnover(epv_ctx *c, uint64_t *hist, uint64_t *len_sum, uint64_t *edges) {
  return c ? part_get(c, kTurnoverPart, c->to, hist, len_sum, edges) : EPV_ERR_ARG;
}

// ---- change tracts (epv_tracts.h)
EPV_API int epv_set_change_tracts(epv_ctx *c, uint64_t max_samples) {
  if (!max_samples) return layer_set_off(c, kTracts);
  if (const int frc = refuse_fixed(c, kTracts)) return frc;
  if (max_samples > EPV_TRACT_MAX_SAMPLES) return fail(c, EPV_ERR_ARG, "change tracts take at most 2^21 samples");
  const int rc = check_ready(c, false);
  if (rc) return rc;
  c->tr.on = true;
  c->tr.max = max_samples;
  return layer_set_on(c, kTracts, tracts_alloc);
}

EPV_API int epv_reset_change_tracts(epv_ctx *c) { return c ? part_reset(c, kTractsPart, c->tr) : EPV_ERR_ARG; }

EPV_API int epv_accumulate_change_tracts(epv_ctx *c) { return layer_accumulate(c, kTracts); }

EPV_API int epv_change_tracts_samples(epv_ctx *c, uint64_t *n) { return part_samples(c, c ? &c->tr : nullptr, n); }

EPV_API int epv_change_tracts_layout(epv_ctx *c, uint32_t *n_branches, uint32_t *n_classes, uint32_t *n_bins, uint64_t *first,
                                     uint64_t *count, uint64_t *chunk_sites) {
  if (!c || !n_branches || !n_classes || !n_bins || !first || !count || !chunk_sites) return EPV_ERR_ARG;
  *n_branches = *n_classes = *n_bins = 0;
  *first = *count = *chunk_sites = 0;
  if (!c->tr.on) return EPV_OK;
  const int rc = part_layout_entry(c, kTractsPart, c->tr);
  if (rc) return rc;
  *n_branches = c->tr.shape.rows / 2u;
  *n_classes = EPV_TRACT_CLASSES;
  *n_bins = EPV_DOM_BINS;
  *first = c->tr.at.lo;
  *count = c->tr.at.cnt;
  *chunk_sites = 64ull * EPV_DOM_CHUNK_WORDS;
  return EPV_OK;
}

EPV_API int epv_get_change_tracts(epv_ctx *c, uint64_t *hist, uint64_t *len_sum, uint64_t *edges) {
  return c ? part_get(c, kTractsPart, c->tr, hist, len_sum, edges) : EPV_ERR_ARG;
}

// ---- spatial correlations (epv_corr.h)
EPV_API int epv_set_spatial_correlation(epv_ctx *c, uint32_t max_lag, uint64_t max_samples) {
  if (!max_lag) return layer_set_off(c, kCorr);
  if (const int frc = refuse_fixed(c, kCorr)) return frc;
  if (!c) return EPV_ERR_ARG;
  if (max_lag > EPV_CORR_MAX_LAG) return fail(c, EPV_ERR_ARG, "spatial correlations take lags up to 1024");
  if (!max_samples) return fail(c, EPV_ERR_ARG, "spatial correlations: max_samples is at least 1");
  if (max_samples > EPV_CORR_MAX_SAMPLES) return fail(c, EPV_ERR_ARG, "spatial correlations take at most 2^21 samples");
  const int rc = check_ready(c, false);
  if (rc) return rc;
  c->co.L = max_lag;
  c->co.max = max_samples;
  return layer_set_on(c, kCorr, corr_alloc);
}

EPV_API int epv_reset_spatial_correlation(epv_ctx *c) { return c ? part_reset(c, kCorrPart, c->co) : EPV_ERR_ARG; }

EPV_API int epv_accumulate_spatial_correlation(epv_ctx *c) { return layer_accumulate(c, kCorr); }

EPV_API int epv_spatial_correlation_samples(epv_ctx *c, uint64_t *n) { return part_samples(c, c ? &c->co : nullptr, n); }

EPV_API int epv_spatial_correlation_layout(epv_ctx *c, uint32_t *n_rows, uint32_t *max_lag, uint64_t *first,
                                           uint64_t *count, uint64_t *chunk_sites) {
  if (!c || !n_rows || !max_lag || !first || !count || !chunk_sites) return EPV_ERR_ARG;
  *n_rows = *max_lag = 0;
  *first = *count = *chunk_sites = 0;
  if (!corr_on(c)) return EPV_OK;
  const int rc = part_layout_entry(c, kCorrPart, c->co);
  if (rc) return rc;
  *n_rows = c->co.shape.rows;
  *max_lag = c->co.L;
  *first = c->co.at.lo;
  *count = c->co.at.cnt;
  *chunk_sites = 64ull * EPV_CORR_CHUNK_WORDS;
  return EPV_OK;
}

EPV_API int epv_get_spatial_correlation(epv_ctx *c, uint64_t *n11, uint64_t *edges) {
  return c ? part_get(c, kCorrPart, c->co, n11, nullptr, edges) : EPV_ERR_ARG;
}

// ---- domain maps (epv_dmaps.h)
EPV_API int epv_set_domain_maps(epv_ctx *c, uint32_t n_sizes, const uint32_t *sizes, uint32_t state, uint64_t max_samples) {
  if (!n_sizes) return layer_set_off(c, kDmaps);
  if (const int frc = refuse_fixed(c, kDmaps)) return frc;
  if (!c) return EPV_ERR_ARG;
  if (!sizes) return fail(c, EPV_ERR_ARG, "null sizes");
  if (n_sizes > EPV_DMAPS_MAX_SIZES) return fail(c, EPV_ERR_ARG, "domain maps take at most 4 sizes");
  for (uint32_t k = 0; k < n_sizes; ++k) {
    if (sizes[k] < 1u || sizes[k] > EPV_DMAPS_MAX_SIZE) return fail(c, EPV_ERR_ARG, "domain maps take sizes 1 .. 1024");
    if (k && sizes[k] <= sizes[k - 1u]) return fail(c, EPV_ERR_ARG, "domain maps take strictly increasing sizes");
  }
  if (state > 1u) return fail(c, EPV_ERR_ARG, "domain maps: the state is 0 or 1");
  if (!max_samples) return fail(c, EPV_ERR_ARG, "domain maps: max_samples is at least 1");
  if (max_samples > EPV_DMAPS_MAX_SAMPLES) return fail(c, EPV_ERR_ARG, "domain maps take at most 2^21 samples");
  const int rc = check_ready(c, false);
  if (rc) return rc;
  c->dp.Z = EpvDmapSizes{};
  c->dp.Z.K = n_sizes;
  for (uint32_t k = 0; k < n_sizes; ++k) c->dp.Z.L[k] = sizes[k];
  c->dp.state = state;
  c->dp.max = max_samples;
  return layer_set_on(c, kDmaps, dmaps_alloc);
}

EPV_API int epv_reset_domain_maps(epv_ctx *c) { return c ? part_reset(c, kDmapsPart, c->dp) : EPV_ERR_ARG; }

EPV_API int epv_accumulate_domain_maps(epv_ctx *c) { return layer_accumulate(c, kDmaps); }

EPV_API int epv_domain_maps_samples(epv_ctx *c, uint64_t *n) { return part_samples(c, c ? &c->dp : nullptr, n); }

EPV_API int epv_domain_maps_layout(epv_ctx *c, uint32_t *n_nodes, uint32_t *n_sizes, uint32_t *sizes, uint32_t *state,
                                   uint64_t *first, uint64_t *count, uint64_t *chunk_sites) {
  if (!c || !n_nodes || !n_sizes || !sizes || !state || !first || !count || !chunk_sites) return EPV_ERR_ARG;
  *n_nodes = *n_sizes = *state = 0;
  for (uint32_t k = 0; k < EPV_DMAPS_MAX_SIZES; ++k) sizes[k] = 0;
  *first = *count = *chunk_sites = 0;
  if (!dmaps_on(c)) return EPV_OK;
  const int rc = part_layout_entry(c, kDmapsPart, c->dp);
  if (rc) return rc;
  *n_nodes = c->dp.shape.rows;
  *n_sizes = c->dp.Z.K;
  for (uint32_t k = 0; k < c->dp.Z.K; ++k) sizes[k] = c->dp.Z.L[k];
  *state = c->dp.state;
  *first = c->dp.at.lo;
  *count = c->dp.at.cnt;
  *chunk_sites = 64ull * EPV_DMAPS_CHUNK_WORDS;
  return EPV_OK;
}

EPV_API int epv_get_domain_maps(epv_ctx *c, uint32_t *counts, uint64_t *edges) {
  return c ? part_get(c, kDmapsPart, c->dp, counts, nullptr, edges) : EPV_ERR_ARG;
}

EPV_API int epv_window_counts_to_stats(epv_ctx *c, const int64_t *counts, uint64_t n_windows, uint64_t samples,
                                       double *J, double *D) {
  if (!c || !counts || !J || !D || !samples) return EPV_ERR_ARG;
  if (!c->have_tree) return fail(c, EPV_ERR_STATE, "epv_set_tree must come first");
  HIP_TRY(c, hipSetDevice(c->device));
  const int rc = ensure_stat_scale(c);     // k_b depends on the genome length and the branch lengths
  if (rc) return rc;
  const uint32_t B = c->S.B;
  const double ns = (double)samples;
  for (uint64_t w = 0; w < n_windows; ++w)
    for (uint32_t b = 0; b < B; ++b) {
      const double inv = 1.0 / c->statscale[b + 1u];     // a power of two: exact
      const int64_t *p = counts + (w * B + b) * 16u;
      for (int k = 0; k < 8; ++k) {
        J[(w * B + b) * 8u + k] = (double)p[k] / ns;
        D[(w * B + b) * 8u + k] = (double)p[8 + k] * inv / ns;
      }
    }
  return EPV_OK;
}

// ---- epoch statistics (epv_epochs.h)
EPV_API int epv_set_epoch_stats(epv_ctx *c, uint32_t P) {
  if (!P) return layer_set_off(c, kEpochs);
  if (const int frc = refuse_fixed(c, kEpochs)) return frc;
  if (P > EPV_EPOCH_MAX_P) return fail(c, EPV_ERR_ARG, "epoch statistics take at most EPV_EPOCH_MAX_P = 256 epochs");
  if (!c) return EPV_ERR_ARG;
  if (!c->have_tree) return fail(c, EPV_ERR_STATE, "epv_set_tree must come first");
  c->ep.P = P;
  return layer_set_on(c, kEpochs, epoch_alloc);
}

EPV_API int epv_reset_epoch_stats(epv_ctx *c) {
  const int rc = layer_entry(c, kEpochs);
  if (rc) return rc;
  if (c->ep.d) HIP_TRY(c, hipMemsetAsync(c->ep.d, 0, (size_t)256u * c->ep.B * c->ep.P, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->ep.samples = 0;
  c->ep.addends = 0;
  c->ep.scale.clear();
  c->ep.fixT.clear();
  return EPV_OK;
}

EPV_API int epv_accumulate_epoch_stats(epv_ctx *c) { return layer_accumulate(c, kEpochs); }

EPV_API int epv_epoch_stats_samples(epv_ctx *c, uint64_t *n) {
  if (!c || !n) return EPV_ERR_ARG;
  *n = c->ep.samples;   // (0 while the layer is off)
  return EPV_OK;
}

EPV_API int epv_epoch_stats_set_samples(epv_ctx *c, uint64_t n) {
  int rc = layer_entry(c, kEpochs);
  if (rc) return rc;
  if (n && c->ep.scale.empty()) {   // (as if the samples had been taken with the scales of now)
    if ((rc = ensure_stat_scale(c))) return rc;
    epoch_remember(c);
  }
  c->ep.samples = n;
  c->ep.addends = n * epoch_blocks(c);   // (as if every one had been taken over the sites of now)
  if (!n) { c->ep.scale.clear(); c->ep.fixT.clear(); }
  return EPV_OK;
}

EPV_API int epv_epoch_stats_layout(epv_ctx *c, uint32_t *B, uint32_t *P, int *k, uint64_t *fixT) {
  if (!c || !B || !P) return EPV_ERR_ARG;
  *B = *P = 0;
  if (!c->ep.P) return EPV_OK;
  if (!c->have_tree) return fail(c, EPV_ERR_STATE, "epv_set_tree must come first");
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->ep.samples == 0) {   // lay out for the tree as it is now
    const int rc = ensure_epochs(c);
    if (rc) return rc;
  }
  const std::vector<double> &sc = c->ep.scale.empty() ? c->statscale : c->ep.scale;
  *B = c->ep.B;
  *P = c->ep.P;
  for (uint32_t b = 1; b <= c->ep.B && b < sc.size(); ++b) {
    if (k) k[b - 1u] = std::ilogb(sc[b]);                                   // (sc[b] = 2^k_b exactly)
    if (fixT) fixT[b - 1u] = c->ep.fixT.empty() ? (uint64_t)std::llrint(c->blen[b] * sc[b]) : c->ep.fixT[b];
  }
  return EPV_OK;
}

EPV_API int epv_get_epoch_stats(epv_ctx *c, uint64_t *raw) {
  const int rc = layer_entry(c, kEpochs);
  if (rc) return rc;
  if (!raw) return fail(c, EPV_ERR_ARG, "null output");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const size_t bytes = (size_t)256u * c->ep.B * c->ep.P;
  if (bytes) HIP_TRY(c, hipMemcpy(raw, c->ep.d, bytes, hipMemcpyDeviceToHost));
  return EPV_OK;
}
