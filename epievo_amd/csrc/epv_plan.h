// epv_plan.h -- what a colour phase runs, decided on the host as pure functions: the launch shapes of the proposal
// kernels (plan_shapes) and the kernel variants under the knobs and the options (phase_plan).  Plain C++17, no HIP
// type, no context: epv_abi.hip keeps and launches what they return, libepv_host.so answers without a GPU
// (epvh_phase_plan).  Include epievo_mi355x.h first: the plan is reported in its EPV_PLAN_* fields.
#ifndef EPV_PLAN_H
#define EPV_PLAN_H

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "epv_device.h"

// The library's knobs: environment variables that a context reads once, when epv_create makes it.
// Each reaches a kernel path that the automatic choice would not take on a test's small input.  In
// brackets, the tests that set it: P test_gpu_parity, M test_kernel_matrix, F test_fused_small_tree,
// A test_path_average_gpu.
//   EPV_PROPOSE_V1=1        the first proposal kernel everywhere [P M]
//   EPV_PROPOSE_V3=0/1      the large-tree proposal kernel never / wherever the plan allows it; default:
//                           where the second kernel's record pool does not fit LDS [P M]
//   EPV_SEG_JUMPS=0/1       segment-parallel jump kernels off / on; default: kbar >= 0.25 [P M A]
//   EPV_FUSED_PHASE=0/1     the fused colour phase off / on; default: phases of <= 3072 waves [P M F A]
//   EPV_P2_SMALL_TREE=0     the fused phase's generic body also on trees of <= EPV_P2_SMALL_MAX nodes [F]
//   EPV_FUSED_LANES=4/8/16/32/64   sites per wave of the fused phase (any other value: 64); default:
//                           by launch size [F]
//   EPV_FORCE_LDS_POOL      (set) the record pool in LDS wherever one lane's worst case fits [P M]
//   EPV_FORCE_GLOBAL_POOL   (set) no LDS record pool: the first kernel's goes to global memory, and
//                           the second kernel is not planned [M]
//   EPV_P3_MIN_LIST         (set) the large-tree kernel's heavy list holds one lane's worst case only,
//                           so that busy waves run in several rounds [P]
//   EPV_P3_SLAB_POOL=0/1/2  the large-tree kernel's slabs: one per block / from a per-XCD pool when the
//                           launch has more blocks than the pool has slabs (default) / always pooled [P M]
//   EPV_ACCEPT_V3=0/1       the accept stage: the (no-)cache kernel / epv_mh_accept3_kernel; default:
//                           accept3 where there is no meta cache [P]
//   EPV_ACCEPT_NO_CACHE     (set) no LDS meta cache in the accept stage [P]
struct EpvKnobs {
  bool propose_v1 = false;
  int propose_v3 = -1;         // -1: by the plan
  int seg_jumps = -1;          // -1: by workload
  int fused_phase = -1;        // -1: by launch size
  bool small_tree = true;
  uint32_t fused_lanes = 0;    // 0: by launch size
  bool force_lds_pool = false, force_global_pool = false;
  bool p3_min_list = false;
  int p3_slab_pool = 1;
  int accept_v3 = -1;          // -1: by the meta cache
  bool accept_no_cache = false;
};

// the knobs as `lookup` holds them: the value of a name, or null where it is not set (epv_create: std::getenv)
template <class Lookup>
EpvKnobs read_knobs(Lookup lookup) {
  EpvKnobs k;
  auto has = [&](const char *name) { return lookup(name) != nullptr; };
  auto num = [&](const char *name, int unset) { const char *e = lookup(name); return e ? std::atoi(e) : unset; };
  k.propose_v1 = num("EPV_PROPOSE_V1", 0) != 0;
  if (has("EPV_PROPOSE_V3")) k.propose_v3 = num("EPV_PROPOSE_V3", 0) != 0 ? 1 : 0;
  if (has("EPV_SEG_JUMPS")) k.seg_jumps = num("EPV_SEG_JUMPS", 0) != 0 ? 1 : 0;
  if (has("EPV_FUSED_PHASE")) k.fused_phase = num("EPV_FUSED_PHASE", 0) != 0 ? 1 : 0;
  k.small_tree = num("EPV_P2_SMALL_TREE", 1) != 0;
  if (has("EPV_FUSED_LANES")) {
    const int v = num("EPV_FUSED_LANES", 0);
    k.fused_lanes = (v == 4 || v == 8 || v == 16 || v == 32 || v == 64) ? (uint32_t)v : 64u;
  }
  k.force_lds_pool = has("EPV_FORCE_LDS_POOL");
  k.force_global_pool = has("EPV_FORCE_GLOBAL_POOL");
  k.p3_min_list = has("EPV_P3_MIN_LIST");
  k.p3_slab_pool = num("EPV_P3_SLAB_POOL", 1);
  k.accept_v3 = num("EPV_ACCEPT_V3", -1);
  k.accept_no_cache = has("EPV_ACCEPT_NO_CACHE");
  return k;
}

// what the launch shapes depend on: the tree in pre-order (host arrays [N], valid as epv_set_tree checks them), the
// jump capacity, the local sites and the mean jumps per (site, branch) of the paths
struct PlanInput {
  uint32_t N;
  const uint32_t *parent, *subtree;
  uint32_t C;
  uint64_t n_sites;
  double kbar;
};
// most sites of one colour phase
inline uint64_t epv_phase_cap(uint64_t n_sites) { return (n_sites + 2u) / 3u + 1u; }
// a counter shard's region of a work list: the worst case of the blocks that use it, `per_site` entries a site
inline uint64_t epv_task_cap(uint64_t n_sites, uint64_t per_site) {
  return ((((n_sites + 2u) / 3u + 63u) / 64u + EPV_SHARDS - 1u) / EPV_SHARDS + 1u) * 64u * per_site;
}
// the fused phase's lists, entries per wave: every branch of 64 sites with 2C+1 segments; a word per branch
inline uint64_t epv_fused_seg_cap(uint32_t B, uint32_t C) { return 64ull * B * (2u * C + 1u); }
inline uint64_t epv_fused_bt_cap(uint32_t B) { return 64ull * B; }
inline size_t const_lds_bytes(uint32_t N) { return (size_t)((20u + N + 1u) & ~1u) * 8u; }
// typical: K = 1 + Poisson(lam) segments per branch, lam = 2 kbar; heavy segments E[K; K >= 2]
inline double heavy_per_branch(double lam) { return (1.0 + lam) - std::exp(-lam); }
inline bool seg_jumps_on(const EpvKnobs &knobs, double kbar) { return knobs.seg_jumps < 0 ? kbar >= 0.25 : knobs.seg_jumps != 0; }
// LDS pool of the second kernel relative to the typical demand: 1.25 -> 1.15 with the 8-double records
// gave one more wave per CU, ~4 % of the waves take a second round
constexpr double P2_MARGIN = 1.15;
// the fused phase pays while a phase has at most this many waves: measured on tree.nwk, +46 % at 520
// waves, +20 % at 1700, +5 % at 2600, -4..-14 % at 5200 (tools/fused_scan.sh)
constexpr uint64_t FUSED_MAX_WAVES = 3072u;

// ---- the launch shapes, one value per proposal kernel
struct PlanV1 {                // epv_mh_propose_kernel
  uint32_t threads = 64, pool_entries = 0;
  bool gpool = false;          // the record pool in global memory (large trees)
  size_t lds = 0;
  uint64_t slab_need = 0;      // doubles of that pool; allocated when a launch first takes the kernel
};
struct PlanV2 {                // epv_mh_propose2_kernel, one wave per block, and the fused phase in its buffers
  bool planned = false;        // the pool fits LDS (otherwise the kernel is not planned)
  uint32_t pool = 0;           // LDS doubles per wave
  size_t lds = 0;
  bool fused = false;          // the fused colour phase: one kernel per phase for launches of few waves
  uint32_t fused_lanes = 64;   // its sites per wave (64 / 32 / 16 by launch size)
};
struct PlanV3 {                // epv_mh_propose3_kernel; default-constructed: not taken
  bool taken = false;
  uint32_t words = 0, list_cap = 0, qrows = 0, n_up = 0, depth = 0;   // (words per node mask)
  uint32_t slots = 0;          // slabs per XCD handed out to resident blocks (0 = a slab per block of the launch)
  size_t lds = 0;
  uint64_t slab_need = 0;      // doubles; allocated when a launch first takes the kernel
  std::vector<uint32_t> nodetab;   // node words and level lists of the kernel (EPV_P3_*), at most 2048 words
};
struct PhaseShapes {
  const char *error = nullptr;   // set: EPV_ERR_ARG with this text, and the shapes hold nothing
  PlanV1 v1;
  PlanV2 v2;
  PlanV3 v3;
};

// choose the MH launch shape: one wave per block; the record pool is as large as fits
// six blocks per CU, but never smaller than one lane's worst case
// (plan_mh and plan_p2 fill a default-constructed value; false: the tree is too large for the node table)
inline bool plan_mh(const PlanInput &in, const EpvKnobs &knobs, PlanV1 &v) {
  const uint32_t N = in.N, B = N - 1u, C = in.C;
  const uint64_t worst = (uint64_t)B * (2u * C + 2u);
  // per wave: node table N*64 u32 (rounded to 16 B) + pool of 16-byte records
  const size_t fixed = const_lds_bytes(N) + (((size_t)N * 64u * 4u + 15u) & ~(size_t)15u);
  if (fixed > 150u * 1024u) return false;
  // typical demand of 64 lanes: B * (2 kbar + 2) records each, with a 30 % margin
  const uint64_t typical = (uint64_t)(64.0 * B * (2.0 * in.kbar + 2.0) * 1.3) + 32u;
  const uint64_t max_fit = fixed + 16u < 160u * 1024u ? (160u * 1024u - fixed) / 16u : 0u;
  const uint64_t want = std::max<uint64_t>(worst, typical);
  // LDS pool while it leaves >= 8 waves per CU (2 per SIMD); otherwise a global-memory slab
  // per block (the working set of the resident waves stays in L2 / Infinity Cache)
  const bool lds_ok = want <= max_fit && (fixed + std::min(want, max_fit) * 16u) * 8u <= 160u * 1024u;
  const bool use_lds = knobs.force_global_pool ? false : knobs.force_lds_pool ? want <= max_fit : lds_ok;
  if (use_lds) {
    const uint64_t pool = std::min(want, max_fit);
    v.pool_entries = (uint32_t)pool;
    v.lds = fixed + (size_t)pool * 16u;
  } else {
    // global slab: `worst` ROWS of 64 interleaved records per wave (a lane can always run)
    const uint64_t blocks = (epv_phase_cap(in.n_sites) + 63u) / 64u;
    v.slab_need = blocks * worst * 128u;
    v.gpool = true;
    v.pool_entries = (uint32_t)worst;
    v.lds = fixed;
  }
  return true;
}

// doubles of a heavy-segment record in a variant of epv_mh_propose2_kernel: 10 in the second kernel when it lists
// segments for the segment-parallel jump kernels (they read the records back), 8 in every fused body and in the
// second kernel otherwise
inline uint32_t p2_hrec(bool fused_body, bool seg) { return !fused_body && seg ? EPV_HREC : EPV_HREC_SHORT; }
// ... and the largest of any variant phase_plan can launch in one pool.  The options are not known when the pool is
// planned, and under EPV_OPT_DIRECT_SAMPLER without EPV_OPT_DIRECT_FUSED the second kernel runs in a pool planned
// next to a fused body; it lists segments exactly when seg_jumps_on says so for these knobs and this kbar.
inline uint32_t p2_hrec_max(const EpvKnobs &knobs, double kbar) { return p2_hrec(false, seg_jumps_on(knobs, kbar)); }
// one lane's worst case in pool doubles: every branch with 2C+1 segments (records K+1 of 2 doubles, heavy K).  A pool
// below it for the launched variant never lets that lane run: launch_fused and launch_propose refuse such a launch.
inline uint64_t p2_worst_dbl(uint32_t B, uint32_t C, uint32_t hrec) {
  return 2u * (uint64_t)B * (2u * C + 2u) + (uint64_t)hrec * B * (2u * C + 1u);
}

// launch shape of epv_mh_propose2_kernel: per wave the constants, the matrix table, the node
// table and a pool of doubles shared by the Felsenstein records (2 doubles) and the heavy-segment
// records (p2_hrec doubles).  The pool covers the typical demand of 64 lanes with a margin (a wave that
// needs more runs in rounds) and always one lane's worst case.
inline bool plan_p2(const PlanInput &in, const EpvKnobs &knobs, PlanV2 &v) {
  const uint32_t N = in.N, B = N - 1u, C = in.C;
  const uint64_t phase_cap = epv_phase_cap(in.n_sites);
  const size_t shared = const_lds_bytes(N) + (size_t)B * 4u * 6u * 8u;     // constants, matrix table: once per block
  const size_t per_wave_fixed = ((((size_t)N * 64u + 1u) / 2u + 1u) & ~(size_t)1u) * 8u +
                                ((3u * 64u + 2u) * (size_t)B * sizeof(epv_meta_t) + 15u) / 16u * 16u;   // node table, meta cache (+ 2 edge columns)
  const size_t fixed = shared + per_wave_fixed;
  // the fused phase: few waves (a launch that leaves SIMDs idle pays one wave chain instead of
  // three to five), at most 64 segments per branch (the hand-over's bit word), lists for the worst
  // case of every wave within 4 GB
  // sites per wave: halve while every SIMD could still get two waves
  uint32_t f_lanes = knobs.fused_lanes ? knobs.fused_lanes : 64u;
  if (!knobs.fused_lanes)
    while (f_lanes > 16u && (phase_cap + f_lanes / 2u - 1u) / (f_lanes / 2u) <= 2048u) f_lanes /= 2u;
  const uint64_t phase_waves = (phase_cap + 63u) / 64u;
  const uint64_t f_bytes = (phase_cap + f_lanes - 1u) / f_lanes *
                           (epv_fused_seg_cap(B, C) * (sizeof(EpvSegTask) + sizeof(EpvSegOut)) + epv_fused_bt_cap(B) * 12u);
  // (The options are not consulted: they may change after the paths are planned.  Under EPV_OPT_DIRECT_SAMPLER
  // without EPV_OPT_DIRECT_FUSED phase_plan never launches the fused phase, yet the pool below is sized as if it
  // did -- `fused` stays true next to the separate V2 kernels, and a tree near the LDS limit may go to the global
  // pool or to V1 for a fused body that does not run.  Results do not depend on it; the cost is not measured.
  // With EPV_OPT_DIRECT_FUSED the fused direct bodies run in these very buffers.)
  const bool fused = !knobs.propose_v1 && 2u * C + 1u <= 64u && f_bytes <= (4ull << 30) &&
                     (knobs.fused_phase < 0 ? phase_waves <= FUSED_MAX_WAVES : knobs.fused_phase != 0);
  // heavy-segment records: the largest of any kernel that phase_plan can launch in this pool under any option
  // word (p2_hrec_max) -- a pool below one lane's worst case would leave the kernel's round loop without an end
  const uint64_t hrec = p2_hrec_max(knobs, in.kbar);
  const uint64_t worst_dbl = p2_worst_dbl(B, C, (uint32_t)hrec);
  const double lam = 2.0 * in.kbar;
  uint32_t n_internal = 0;
  for (uint32_t node = 1; node < N; ++node) n_internal += in.subtree[node] != 1u;
  const double rec_per_lane = B * (1.0 + lam) + n_internal;     // K per branch, +1 for an internal node's q
  const uint64_t typical_dbl = (uint64_t)(64.0 * (2.0 * rec_per_lane + (double)hrec * B * heavy_per_branch(lam)) * P2_MARGIN) + 64u;
  const uint64_t max_fit = fixed + 64u < 160u * 1024u ? (160u * 1024u - fixed) / 8u : 0u;
  uint64_t want = std::max(worst_dbl, typical_dbl);
  // the fused phase reuses the pool for the search's cooperative area and then for the accept
  // stage's task table, results, accumulators (992 doubles) and meta words (3 B columns of 64)
  if (fused) want = std::max<uint64_t>(want, std::max<uint64_t>(EPV_COOP_BYTES / 8u, 992u + 48u * (uint64_t)B));
  const bool lds_ok = want <= max_fit && (fixed + want * 8u) * 5u <= 160u * 1024u;   // >= 5 waves per CU
  const bool use_lds = knobs.force_global_pool ? false : knobs.force_lds_pool ? want <= max_fit : lds_ok;
  if (fixed > 150u * 1024u) return false;
  v.planned = use_lds;
  v.fused = fused && use_lds;
  v.fused_lanes = f_lanes;
  v.pool = use_lds ? (uint32_t)((want + 1u) & ~(uint64_t)1u) : 0u;
  v.lds = fixed + (size_t)v.pool * 8u;
  return true;
}

// launch shape of epv_mh_propose3_kernel, for trees whose record pool does not fit LDS: per wave a
// 16-bit word per (node, lane) and a stack of partial products in LDS, q rows of the internal nodes
// and the heavy-segment records in a slab of global memory.  A tree or a size the kernel does not take: {}
inline PlanV3 plan_p3(const PlanInput &in, const EpvKnobs &knobs, const PlanV2 &v2) {
  const uint32_t N = in.N, B = N - 1u, C = in.C;
  if (knobs.propose_v3 == 0 || knobs.propose_v1 || N > 128u || N < 2u) return {};     // (node masks of one or two 64-bit words)
  if (knobs.propose_v3 < 0 && v2.planned) return {};     // the LDS pool is the better place while it fits
  // per node: parent, children, depth; q rows for the internal nodes below the root
  std::vector<uint32_t> depth(N, 0u), c1(N, 0u), c2(N, 0u), kids(N, 0u), qrow(N, 0u);
  uint32_t qrows = 0, max_depth = 0;
  for (uint32_t node = 1; node < N; ++node) {
    const uint32_t par = in.parent[node];
    if (par >= node) return {};                          // (pre-order is what epv_set_tree checks; be safe)
    depth[node] = depth[par] + 1u;
    max_depth = std::max(max_depth, depth[node]);
    if (kids[par] == 0u) c1[par] = node; else if (kids[par] == 1u) c2[par] = node;
    ++kids[par];
  }
  for (uint32_t node = 1; node < N; ++node) {
    if (kids[node] > 2u) return {};                      // two child fields per node word
    if (in.subtree[node] != 1u) qrow[node] = qrows++;
  }
  if (qrows > 63u) return {};                            // (six bits in the node word; at N <= 128 only unary nodes reach it)
  // tables: node words [N] | internal nodes deepest first [n_up] | their level starts [D + 2] |
  //         all nodes but the root by depth [N - 1] | their level starts [D + 2]
  PlanV3 v;
  std::vector<uint32_t> &tab = v.nodetab;
  for (uint32_t node = 0; node < N; ++node)
    tab.push_back(in.parent[node] | (c1[node] << 7) | (c2[node] << 14) | (qrow[node] << 21) |
                  ((in.subtree[node] == 1u ? 1u : 0u) << 27));
  std::vector<uint32_t> up, upstart(max_depth + 2u, 0u), dn, dnstart(max_depth + 2u, 0u);
  for (uint32_t d = max_depth + 1u; d-- > 0u;) {        // upstart[d + 1] .. upstart[d] = internal nodes of depth d
    if (d <= max_depth && d >= 1u)
      for (uint32_t node = 1; node < N; ++node)
        if (depth[node] == d && in.subtree[node] != 1u) up.push_back(node);
    upstart[d] = (uint32_t)up.size();
  }
  upstart[max_depth + 1u] = 0u;
  for (uint32_t d = 0; d <= max_depth; ++d) {           // dnstart[d] .. dnstart[d + 1] = nodes of depth d
    dnstart[d] = (uint32_t)dn.size();
    if (d >= 1u)
      for (uint32_t node = 1; node < N; ++node)
        if (depth[node] == d) dn.push_back(node);
  }
  dnstart[max_depth + 1u] = (uint32_t)dn.size();
  tab.insert(tab.end(), up.begin(), up.end());
  tab.insert(tab.end(), upstart.begin(), upstart.end());
  tab.insert(tab.end(), dn.begin(), dn.end());
  tab.insert(tab.end(), dnstart.begin(), dnstart.end());
  for (uint32_t g = 0; g < max_depth; ++g) {            // pair groups: leaves, then internal nodes by depth
    uint64_t m = 0, m2 = 0;      // nodes 0..63, 64..127
    for (uint32_t node = 1; node < N; ++node) {
      const bool leaf = in.subtree[node] == 1u;
      if (g == 0u ? leaf : (!leaf && depth[node] == g)) (node < 64u ? m : m2) |= 1ull << (node & 63u);
    }
    tab.push_back((uint32_t)m);
    tab.push_back((uint32_t)(m >> 32));
    tab.push_back((uint32_t)m2);
    tab.push_back((uint32_t)(m2 >> 32));
  }
  for (uint32_t node = 0; node < N; ++node) tab.push_back(depth[node]);
  const uint64_t worst_heavy = (uint64_t)B * (2u * C + 1u);
  // EPV_P3_MIN_LIST=1 (tests): one lane's worst case only, so that busy waves run in several rounds
  const uint64_t list_cap = knobs.p3_min_list ? worst_heavy
                          : std::max<uint64_t>(worst_heavy, (uint64_t)(64.0 * B * heavy_per_branch(2.0 * in.kbar) * 1.5) + 64u);
  if (list_cap >= (1ull << 20)) return {};                 // the pair word's record field
  // a pool of slabs per XCD, claimed by resident blocks (EPV_P3_SLAB_POOL=0: one per block of the launch):
  // 4 blocks of this kernel fit a CU (LDS) and an XCD of the MI355X has 32 CUs: 128 resident blocks at most,
  // 160 slabs per XCD.  Used when the launch has more blocks than the pool has slabs (EPV_P3_SLAB_POOL=2: always)
  const int pool_env = knobs.p3_slab_pool;
  const uint64_t launch_waves = ((epv_phase_cap(in.n_sites) + 255u) / 256u) * 4u;
  v.slots = (pool_env == 2 || (pool_env && launch_waves > 8u * 160u * 4u)) ? 160u : 0u;
  const uint64_t waves = v.slots ? 8ull * v.slots * 4u : launch_waves;
  v.slab_need = waves * ((uint64_t)qrows * 128u + list_cap * EPV_HREC_SHORT);
  if (v.slab_need * sizeof(double) > (24ull << 30)) return {};
  if (tab.size() > 2048u) return {};
  const size_t shared = const_lds_bytes(N) + (size_t)B * 4u * EPV_SEGTAB_DBL * 8u + (tab.size() + 1u) / 2u * 8u;
  const size_t per_wave = ((size_t)EPV_P3_PCAP * 3u + EPV_P3_PCAP / 8u + (max_depth * 64u * 2u + 7u) / 8u + (max_depth + 3u) / 2u) * 8u;   // pair list, pair results, group offsets
  v.lds = shared + 4u * per_wave;
  if (v.lds > 120u * 1024u) return {};        // (a very deep tree's group offsets: keep the first kernels)
  v.words = N > 64u ? 2u : 1u;
  v.list_cap = (uint32_t)list_cap;
  v.qrows = qrows;
  v.n_up = (uint32_t)up.size();
  v.depth = max_depth;
  v.taken = true;
  return v;
}

// the launch shapes of every proposal kernel, for a tree, its paths and their capacity
inline PhaseShapes plan_shapes(const PlanInput &in, const EpvKnobs &knobs) {
  PhaseShapes s;
  if (plan_mh(in, knobs, s.v1) && plan_p2(in, knobs, s.v2)) s.v3 = plan_p3(in, knobs, s.v2);
  else s.error = "tree too large for the 160 KiB LDS node table";
  return s;
}

// the kernel variants of a colour phase (EPV_PLAN_* fields of include/epievo_mi355x.h): launch_phase
// launches what this says, epv_phase_plan and epv_phase_mode report it
struct PhasePlan {
  uint32_t propose;      // EPV_PLAN_V1 / V2 / V3 / FUSED
  bool gpool;            // V1: the record pool in global memory
  bool refq;             // the proposal ratio is evaluated (V1 takes the reference template)
  uint32_t small_nn;     // fused: the small-tree body's node count, 0 = generic body
  uint32_t p3_words;     // V3: words per node mask
  bool p3_slab_pool;     // V3: slabs from the per-XCD pool
  uint32_t jumps;        // EPV_PLAN_JUMPS_*
  uint32_t accept;       // EPV_PLAN_ACCEPT_*
  bool listed;           // the accept stage reads the listed sites
  bool meta_cache;       // (accept and fused kernels) the LDS meta cache
  bool unobs;            // a leaf cell is unobserved: V1 takes the template that marginalises it
  bool evidence;         // a leaf cell carries evidence: V1 takes the template that reads the table
                         // (beside V2, V3 or FUSED, under EPV_OPT_LEAF_FAST: the leaf variant of that kernel)
  uint32_t lanes_log2;   // fused: log2 of the sites per wave (2 .. 6)
  bool direct;           // the jump stage's direct variants (EPV_OPT_DIRECT_SAMPLER)
  uint32_t word() const {
    return propose | (gpool ? 1u : 0u) << 2 | (refq && propose == EPV_PLAN_V1 ? 1u : 0u) << 3 | small_nn << 4 |
           p3_words << 8 | (p3_slab_pool ? 1u : 0u) << 10 | jumps << 12 | accept << 14 | (listed ? 1u : 0u) << 16 |
           (unobs ? 1u : 0u) << 17 | (evidence ? 1u : 0u) << 18 | lanes_log2 << 20 | (direct ? 1u : 0u) << 23;
  }
};
inline PhasePlan phase_plan(const PhaseShapes &shapes, const EpvKnobs &knobs, uint32_t flags, uint64_t unobs_cells,
                            uint64_t evidence_cells, uint32_t B, double kbar) {
  PhasePlan P{};
  const uint32_t N = B + 1u;
  // (root resampling changes the proposal's normalising constant with the path: the ratio must be evaluated)
  P.refq = flags & (EPV_FLAG_REFERENCE_PROPOSAL_RATIO | EPV_FLAG_SAMPLE_ROOT);
  // unobserved leaf cells: the first kernel marginalises them
  P.unobs = unobs_cells != 0u;
  // leaf evidence: the same rule
  P.evidence = evidence_cells != 0u;
  // ... unless EPV_OPT_LEAF_FAST is set: the plan is then what the context would get with no
  // cell held, and bits 17 / 18 select the leaf variant of whichever kernel that is
  const bool held = (P.unobs || P.evidence) && !(flags & EPV_FLAG_LEAF_FAST);
  // the reference-arithmetic mode keeps the first kernel, and so do trees whose record pool does
  // not fit LDS: with the pool in global memory the second kernel's extra passes over it cost
  // more than its dense evaluation saves (16-leaf tree: 830 vs 676 us)
  const bool p3 = shapes.v3.taken && !P.refq && !held;
  const bool p2 = !p3 && !knobs.propose_v1 && !P.refq && !held && shapes.v2.planned;
  P.meta_cache = B <= 8u && !knobs.accept_no_cache;
  // the direct sampler: the separate jump-time kernels, and the fused phase's direct
  // bodies only where EPV_OPT_DIRECT_FUSED asks for them
  P.direct = flags & EPV_FLAG_DIRECT_SAMPLER;
  // (the fused direct bodies have no leaf variant: with a held cell the plan is plain direct mode's)
  const bool direct_fused = (flags & EPV_FLAG_DIRECT_FUSED) && !(P.unobs || P.evidence);
  if (p2 && shapes.v2.fused && (!P.direct || direct_fused)) {
    P.propose = EPV_PLAN_FUSED;
    P.small_nn = knobs.small_tree && N >= 2u && N <= EPV_P2_SMALL_MAX ? N : 0u;
    P.jumps = EPV_PLAN_JUMPS_FUSED;
    P.accept = EPV_PLAN_ACCEPT_FUSED;
    for (uint32_t l = shapes.v2.fused_lanes; l > 1u; l >>= 1) ++P.lanes_log2;
    return P;
  }
  if (p3) {
    P.propose = EPV_PLAN_V3;
    P.p3_words = shapes.v3.words;
    P.p3_slab_pool = shapes.v3.slots != 0u;
  } else if (p2) {
    P.propose = EPV_PLAN_V2;
  } else {
    P.propose = EPV_PLAN_V1;
    P.gpool = shapes.v1.gpool;
  }
  // segment-parallel jumps pay on long branches (single branch T = 1: +17 %, every segment is
  // dirty and needs several trials) and cost on short ones (tree.nwk: -12 %, one dirty segment in
  // fourteen branches does not repay the extra hand-over): profiles/r02_ab_seg_jumps.txt
  // The one-segment tasks (the first bucket: ~95 % on short branches) otherwise go to their own lean
  // kernel, epv_mh_jumps_all_kernel.  (Forward-rejection mode keeps the general kernel for
  // everything: a flip there can need 1e5 trials, which only the wave-wide search takes in reasonable time.)
  // (The direct sampler has no lean one-segment body either: the general kernel's direct variant.)
  P.jumps = p2 && seg_jumps_on(knobs, kbar) ? EPV_PLAN_JUMPS_SEGMENTS
          : !(flags & (EPV_FLAG_FORWARD_REJECTION | EPV_FLAG_DIRECT_SAMPLER)) ? EPV_PLAN_JUMPS_ALL : EPV_PLAN_JUMPS_GENERAL;
  // large trees (no room for the meta cache): a lane per (site, triple), branches in groups (epv_accept3.h)
  const int acc_v3 = knobs.accept_v3;
  P.accept = (acc_v3 >= 0 ? acc_v3 != 0 : !P.meta_cache) ? EPV_PLAN_ACCEPT_V3
           : P.meta_cache ? EPV_PLAN_ACCEPT_CACHE : EPV_PLAN_ACCEPT_NO_CACHE;
  P.listed = p2 || p3;
  return P;
}

#endif
