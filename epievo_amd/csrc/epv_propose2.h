#ifndef EPV_PROPOSE2_H
#define EPV_PROPOSE2_H
// epv_propose2.h -- the proposal kernel of a colour phase, second generation (included by
// epv_kernels.h).  Same contract as epv_mh_propose_kernel<., false> -- pruning
// (SingleSiteSampler.cpp:116-157) and downward sampling of the segment end states (:180-255) of
// one site per lane, bit for bit the numbers of the oracle's parallel rung -- reorganised
// around what the lanes of a wave have in common:
//
//  * ~90 % of the (site, branch) pairs on a short tree have ONE segment (no neighbour jump on
//    that branch).  Its transition matrix depends only on (branch, left state, right state):
//    epv_segtab_kernel evaluates the 4 B matrices once per reset (the very expressions of the
//    per-segment code, so the bits are the same) and the lanes read them from LDS -- no exp,
//    no division.
//  * the other ("heavy") branches drove the cost of the first kernel: a wave iterated
//    max_lanes(K) times over exp + divisions although the average lane has 1.1 segments
//    (lane utilisation 44 %, profiles/r02b_pmc_valu_tree.csv).  Here the lanes only LIST their
//    heavy segments (length, context, Philox address) in LDS; the wave then evaluates the list
//    densely, one segment per lane -- matrices, no-jump bounds and the segment's Philox block,
//    none of which depends on the recursion state -- and the two recursions (Felsenstein
//    partials upwards, end states downwards) read finished 64-byte records: their divergent
//    loops are a handful of FMAs (and one division) per iteration.
//  * a proposal that EQUALS the current path on every branch (no jumps on either, same states:
//    ~70 % of the sites of tree.nwk) is accepted with probability one and changes nothing --
//    the likelihoods it would recompute are the cached ones.  Such a site is counted here and
//    never reaches the accept kernel; all other sites are appended to a compact list that
//    epv_mh_accept_kernel walks with dense lanes.
//
// LDS per wave: constants, the matrix table, the node table regA[N][64] (record offset of the
// branch above the node | proposal end state << 31) and a pool of doubles holding, for the
// lanes that run in this round, their Felsenstein records {p0, p1} (K per branch, +1 for the
// q of an internal node) followed by the wave's heavy-segment records.

struct EpvSegRec {      // one segment, everything the recursions need
  double P00, P11;      // continuous_time_trans_prob_mat (pruning form: h = 1 / exp(len (r0 + r1)))
  double PT00, PT10;    // get_trans_prob(len, prev, 0) for prev = 0, 1 (h = exp(-len (r0 + r1)))
  double nb0, nb1;      // no-jump bounds of trial 1 for a segment that waits in state 0 / 1
  double u_end, u_first;  // the segment's Philox block: end-state uniform, trial 1's first draw
  double len;           // segment length (kept for the jump tasks)
  uint64_t info;        // trip0 | owner lane << 3 | node << 9 | k << 21
};

// The two halves of a segment's evaluation, one exponential each.  The fused bodies run them as two passes over
// their 8-double records (pruning reads the first half's values and is done with them before the downward pass
// reads the second half's); everything else takes both through epv_seg_matrices.
// the pruning form: P00, P11
EPV_DEV void epv_seg_prune_matrix(double len, double r0, double r1, double out[2]) {
  const double denom = r0 + r1;
  const double h = 1.0 / epv_exp(len * (r0 + r1));     // ContinuousTimeMarkovModel.cpp:143-161
  out[0] = (r0 * h + r1) / denom;
  out[1] = (r0 + r1 * h) / denom;
}
// the downward pass's: PT00, PT10 and the no-jump bounds
EPV_DEV void epv_seg_sample_matrices(double len, double r0, double r1, double out[4]) {
  const double denom = r0 + r1;
  const double h2 = epv_exp(-len * (r0 + r1));         // :116-125, shared by both start states
  out[0] = gtp(r0, r1, h2, denom, 0u, 0u);
  out[1] = gtp(r0, r1, h2, denom, 1u, 0u);
#if defined(__HIP_DEVICE_COMPILE__)
  out[2] = nojump_bound(len * r0);
  out[3] = nojump_bound(len * r1);
#else
  out[2] = 0.0;
  out[3] = 0.0;
#endif
}
// (host too, for epv_math_kat's host pass: the four matrix entries; the bounds are a device float exp)
// (both halves, written out: the separate kernels' instruction streams are the ones they had before the split)
EPV_DEV void epv_seg_matrices(double len, double r0, double r1, double out[6]) {
  const double denom = r0 + r1;
  const double h = 1.0 / epv_exp(len * (r0 + r1));     // ContinuousTimeMarkovModel.cpp:143-161
  out[0] = (r0 * h + r1) / denom;
  out[1] = (r0 + r1 * h) / denom;
  const double h2 = epv_exp(-len * (r0 + r1));         // :116-125, shared by both start states
  out[2] = gtp(r0, r1, h2, denom, 0u, 0u);
  out[3] = gtp(r0, r1, h2, denom, 1u, 0u);
#if defined(__HIP_DEVICE_COMPILE__)
  out[4] = nojump_bound(len * r0);
  out[5] = nojump_bound(len * r1);
#else
  out[4] = 0.0;
  out[5] = 0.0;
#endif
}

// tab[(b * 4 + 2 * left_state + right_state) * 6 ..]: the single segment of branch b (length =
// the branch length) in each of the four neighbour contexts
__global__ void epv_segtab_kernel(EpvDev S, double *tab) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= S.B * 4u) return;
  const uint32_t b = t >> 2, li = (t >> 1) & 1u, ri = t & 1u;
  const double *rates = reinterpret_cast<const double *>(S.model);
  const uint32_t trip0 = 4u * li + ri;
  const double len = S.blen[b + 1u] - 0.0;
  double m[6];
  epv_seg_matrices(len, rates[trip0], rates[trip0 | 2u], m);
#pragma unroll
  for (int i = 0; i < 6; ++i) tab[(size_t)t * EPV_SEGTAB_DBL + i] = m[i];
}

// Append the dirty (site, branch) pairs of the last <= 64 branches to the task lists of this
// block's shard -- a WAVE-WIDE operation (lanes without dirty bits pass zeros).  Four buckets by
// segment count so that the waves of the jumps kernel, which take consecutive tasks, hold lanes
// with similar loop counts: a shard has two regions, each filled from BOTH ends (counts packed
// lo/hi in one word) -- region 0: K = 1 from the front, K = 2 from the back; region 1: K = 3
// from the front, K >= 4 from the back.  One atomic per wave and region reserves the slots.
// A task word is branch << 40 | site.  A ONE-SEGMENT branch (no neighbour jump) may carry everything the
// jump kernels would otherwise load -- buffer of the proposal, start state, sampled end state, the
// neighbours' start states -- in its upper bits (EPV_TASK_COMPACT, epv_device.h): epv_mh_jumps1_kernel
// then starts its trials one round trip after reading the word.  `compact` marks those branches; selP,
// xstart, xsamp, xL, xR are the values, one bit per branch like `dirty`.
__device__ __forceinline__ void epv_flush_tasks(const EpvDev &S, unsigned long long *counters,
                                                unsigned long long dirty, unsigned long long multi,
                                                unsigned long long deep, uint32_t b, uint64_t site, int lane,
                                                uint32_t shard, unsigned long long compact = 0ull, uint32_t selP = 0u,
                                                unsigned long long xstart = 0ull, unsigned long long xsamp = 0ull,
                                                unsigned long long xL = 0ull, unsigned long long xR = 0ull) {
#pragma unroll
  for (uint32_t reg = 0; reg < 2u; ++reg) {
    const unsigned long long mine_reg = reg ? (dirty & deep) : (dirty & ~deep);
    const uint32_t mineB = (uint32_t)__popcll(mine_reg & multi);
    const uint32_t mineA = (uint32_t)__popcll(mine_reg) - mineB;
    const uint32_t inclA = wave_incl_scan_u32(mineA), inclB = wave_incl_scan_u32(mineB);
    const uint32_t totalA = epv_bcast(inclA, 63), totalB = epv_bcast(inclB, 63);
    if (totalA | totalB) {
      unsigned long long base = 0ull;
      if (lane == 0)
        base = atomicAdd(&counters[EPV_CNT_IDX(reg ? EPV_CNT_TASKS2 : EPV_CNT_TASKS, shard)],
                         (unsigned long long)totalA | ((unsigned long long)totalB << 32));
      const uint32_t baseA = epv_bcast((uint32_t)base, 0), baseB = epv_bcast((uint32_t)(base >> 32), 0);
      unsigned long long *region = S.tasks + ((unsigned long long)shard * 2u + reg) * S.task_cap;
      unsigned long long slotA = (unsigned long long)baseA + (inclA - mineA);
      unsigned long long slotB = S.task_cap - 1ull - ((unsigned long long)baseB + (inclB - mineB));
      unsigned long long d = mine_reg;
      while (d) {
        const uint32_t bit = (uint32_t)(__ffsll((long long)d) - 1);
        d &= d - 1ull;
        unsigned long long t = ((unsigned long long)((b & ~63u) + bit) << 40) | site;
        if ((compact >> bit) & 1ull)
          t |= EPV_TASK_COMPACT | ((unsigned long long)selP << EPV_TASK_SELP_SHIFT) |
               (((xstart >> bit) & 1ull) << EPV_TASK_START_SHIFT) | (((xsamp >> bit) & 1ull) << EPV_TASK_SAMPLED_SHIFT) |
               (((xL >> bit) & 1ull) << EPV_TASK_LINIT_SHIFT) | (((xR >> bit) & 1ull) << EPV_TASK_RINIT_SHIFT);
        if ((multi >> bit) & 1ull) region[slotB--] = t;
        else region[slotA++] = t;
      }
    }
  }
}

#ifndef EPV_PROPOSE2_WAVES
#define EPV_PROPOSE2_WAVES 3
#endif

// -DEPV_P2_PROFILE: wave-time per section of the kernel, read back by tools/p2_profile.py
#ifdef EPV_P2_PROFILE
// one row per wave and plain stores: atomics on shared counters would serialise the waves and
// show up as waiting time wherever the compiler put the next s_waitcnt
#define EPV_P2_PROF_ROWS 8192
__device__ unsigned long long epv_p2_prof[16 * EPV_P2_PROF_ROWS];
#define P2_MARK(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); t_acc_[i] += t_ - t_prev_; t_prev_ = t_; } while (0)
#else
#define P2_MARK(i) do {} while (0)
#endif
// FUSED (small launches, LDS pool only): the wave keeps the segment and branch lists of ITS 64 sites
// in a private region of global memory and runs the whole colour phase itself -- proposal, then
// the segment search, the assembly of its dirty branches and the acceptance of its sites with the
// device functions of epv_seg_search_kernel / epv_seg_assemble_kernel / epv_mh_accept_kernel.
// Every site of a colour is independent of the others, so nothing in a phase needs more than a
// wave; what the separate kernels buy is dense lanes, and what they cost is one ~20 us wave chain
// per kernel, which is all there is to pay when a launch has fewer waves than the chip has SIMDs.
// Who finishes a branch (times and meta word of the proposal): the grouped search's winning lane, for
// a branch whose sole dirty segment it has just settled with at most two jumps and room for them
// (the segment task says so: w3 bits 5, 6); the assembly stage for every branch of the wave
// otherwise -- it is skipped only when the search has finished ALL of the wave's branches.
struct EpvFused {
  EpvSegTask *segs;            // [waves][seg_cap]
  EpvSegOut *outs;             // [waves][seg_cap]
  unsigned long long *bt;      // [waves][bt_cap]
  uint32_t *bfirst;            // [waves][bt_cap]
  uint32_t seg_cap, bt_cap;    // per wave: 64 B (2C+1) and 64 B -- the worst case, so nothing overflows
  uint32_t meta_cache;         // accept stage: meta words of the five columns in LDS (B <= 8)
  uint32_t lanes;              // sites per wave
  uint32_t grouped_rounds;     // rounds of the grouped search of short segment lists (0 = off)
  uint32_t topo;               // small-tree body: the topology word (bit node: a leaf; bits 8 + 3 node ..: the parent)
  unsigned long long *giveups; // DIRECT bodies: the direct sampler's give-up counter (epv_direct_giveups)
};

// NN > 0 (fused phase only): the node count as a compile-time constant, for trees of at most
// EPV_P2_SMALL_MAX nodes (5: from 6 nodes on, the unrolled body spills to scratch at 168 VGPRs).  The
// node loops of the downward pass, the hand-over and the emission listing unroll; the lane's row of the
// node table and one packed word per branch (meta word, K, matrix-table column) live in registers
// indexed by constants, and the topology is one scalar word read at the kernel's head.  The LDS copies
// stay for what other lanes read (heavy-pair merges, the emission pass, the acceptance stage).  Same
// operations in the same order: the results are the generic body's bit for bit.  NN = 0: S.N nodes.
// DIRECT (fused phase only, EPV_OPT_DIRECT_FUSED): the jump stage samples every segment of the wave's list by
// run_direct (epv_direct.h) instead of searching trials -- one counted loop over the list, then the assembly of
// every branch; the searches and their cooperative LDS area are not compiled, so every loop of the kernel is counted.
// LEAF (EPV_OPT_LEAF_FAST): a leaf's q is the leaf vector of LS (epv_leaf_word: evidence, else
// the mask, else the indicator) wherever the body would set it from the current path's end state.  Pruning loads the
// cell's word at the head of the leaf's iteration and files the vector as the branch's record K, like an internal
// node's q (so a leaf branch takes K + 1 records here, which one lane's worst case covers: plan_p2), and the downward
// pass reads it back through the generic p[k + 1].  Nothing else reads the current path's end state: `ident` and the
// clean-branch test compare the PROPOSAL's states with the path's start states and jump counts, and the hand-over's
// end_b is the proposal's sampled end state.  The table and the mask (device layouts of epv_leaf_evidence and
// epv_unobserved, either may be null) are the two trailing arguments only these instantiations take, as with the
// first kernel's: the others keep their argument layout and their instruction streams.
template <bool SEG, bool FUSED, int NN = 0, bool DIRECT = false, class... Leaf>
__global__ __launch_bounds__(256, EPV_PROPOSE2_WAVES) void epv_mh_propose2_kernel(
    EpvDev S, uint32_t colour, uint32_t seed_lo, uint32_t seed_hi, uint32_t sweep, uint64_t first,
    uint64_t last, uint64_t own_first, uint64_t own_last, uint32_t pool_dbl, uint32_t list_cap,
    uint32_t parity, unsigned long long *counters, double *gpool, const double *segtab, EpvFused F, Leaf... leaf_args) {
  constexpr bool LEAF = sizeof...(Leaf) != 0;
  static_assert(sizeof...(Leaf) == (LEAF ? 2u : 0u), "the table and the mask come together");
  [[maybe_unused]] EpvLeafSrc LS{nullptr, nullptr};
  if constexpr (LEAF) { LS.table = epv_first_arg(leaf_args...); LS.mask = epv_second_arg(leaf_args...); }
  static_assert(!FUSED || SEG, "the fused phase emits segments");
  static_assert(!DIRECT || FUSED, "the direct body is the fused phase's");
  static_assert(!LEAF || !DIRECT, "the fused direct bodies have no leaf variant");
  constexpr bool SMALL = NN > 0;
  static_assert(!SMALL || (FUSED && NN >= 2 && NN <= EPV_P2_SMALL_MAX), "the small-tree body is the fused phase's");
  constexpr int NNA = SMALL ? NN : 1;      // register array extents (1: unused by the generic body)
  constexpr int NBA = SMALL ? NN - 1 : 1;
  const uint32_t NNODE = SMALL ? (uint32_t)NN : S.N;
  // SEG: true = dirty SEGMENTS go to the segment-parallel jump kernels (epv_jumps2.h); 0 = dirty
  // branches go to epv_mh_jumps_kernel's bucketed lists
  // pool_dbl: the LDS pool, doubles per wave (records and heavy list share it); list_cap and gpool are unused
  extern __shared__ __attribute__((aligned(16))) double s_mem[];
  // heavy-segment records: 10 doubles only where the segment-parallel jump kernels' hand-over reads length and
  // address word behind all eight fields.  FUSED: 8 -- length and address word keep slots 6 and 7 for the life of
  // the record, and the eight fields come in two passes over slots 0..5 (pruning form, then the downward pass's)
  constexpr uint32_t HREC = (SEG && !FUSED) ? EPV_HREC : EPV_HREC_SHORT, LEN_AT = HREC - 2u, INFO_AT = HREC - 1u;
  // slots of the downward pass's fields: EpvSegRec's order in the separate kernels, pass 2's in the fused bodies
  constexpr uint32_t F_PT = FUSED ? 0u : 2u, F_NB = FUSED ? 2u : 4u, F_UEND = FUSED ? 4u : 6u, F_UFIRST = FUSED ? 5u : 7u;
  // ... and where the downward pass parks a dirty heavy branch's sampled states and its dirty-segment mask for
  // the hand-over: the two uniforms' slots of the branch's first record, used by then
  [[maybe_unused]] constexpr uint32_t F_W64 = F_UEND, F_DMASK = F_UFIRST;
#ifdef EPV_P2_PROFILE
  unsigned long long t_acc_[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  unsigned long long t_prev_ = __builtin_readcyclecounter();
#endif
  const uint32_t B = SMALL ? (uint32_t)NN - 1u : S.B;
  const uint32_t const_dbl = (20u + NNODE + 1u) & ~1u;
  const uint32_t tab_dbl = B * 4u * EPV_SEGTAB_DBL;
  const uint32_t regA_dbl = ((NNODE * 64u + 1u) / 2u + 1u) & ~1u;
  // meta words of the three columns of every lane, + the column two sites left of lane 0 and two
  // sites right of the last lane (the acceptance stage's outer triples; the other lanes' outer
  // columns ARE their neighbour lanes' inner ones: lane l + 1 sits three sites further)
  const uint32_t mc_dbl = ((3u * 64u + 2u) * B * (uint32_t)sizeof(epv_meta_t) + 15u) / 16u * 2u;
  // a block holds blockDim.x / 64 waves: constants and the matrix table once, then per wave the
  // node table, the meta cache and the pool
  const uint32_t wave_id = threadIdx.x >> 6;
  // the counter shard and list regions are per WAVE (as if every wave were its own block)
  const uint32_t my_shard = (blockIdx.x * (blockDim.x >> 6) + wave_id) & (EPV_SHARDS - 1u);
  const uint32_t wave_dbl = regA_dbl + mc_dbl + ((pool_dbl + 1u) & ~1u);
  double *s_const = s_mem;
  double *s_tab = s_mem + const_dbl;
  double *s_wave = s_mem + const_dbl + tab_dbl + (size_t)wave_id * wave_dbl;
  uint32_t *regA = reinterpret_cast<uint32_t *>(s_wave);
  // s_meta[(which * B + b) * 64 + lane], which = 0 left, 1 right, 2 this site: fetched ONCE, in one
  // batch of independent loads; the four passes below then read LDS instead of paying a global
  // round trip per branch (the kernel is bound by memory latency, not by issue)
  epv_meta_t *s_meta = reinterpret_cast<epv_meta_t *>(s_wave + regA_dbl);
  epv_meta_t *s_edge = s_meta + 3u * B * 64u;     // [0 .. B): left of lane 0, [B .. 2B): right of the last valid lane
  const int lane = epv_lane();
  // records packed by a wave prefix sum, the heavy list behind them
  double *pool = s_wave + regA_dbl + mc_dbl;
  const uint64_t gfirst = S.g0 + first;
  const uint64_t s0 = first + ((colour + 3u - (uint32_t)(gfirst % 3u)) % 3u);
  // FUSED: F.lanes (64, 32 or 16) sites per wave -- fewer sites, hence fewer search rounds, per wave
  // when that still leaves SIMDs idle; the other lanes only help in the cooperative stages
  const uint32_t lpw = FUSED ? F.lanes : 64u;
  const uint64_t tid = FUSED ? ((uint64_t)blockIdx.x * (blockDim.x >> 6) + wave_id) * lpw + (uint32_t)(threadIdx.x & 63u)
                             : (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t site = s0 + 3u * tid;
  const bool valid = site <= last && (threadIdx.x & 63u) < lpw;
  const uint64_t n = S.n;
  const uint32_t gsite = (uint32_t)(S.g0 + site);
  const uint32_t gsite_lane0 = gsite - 3u * (uint32_t)lane;

  // the head of the kernel's dependent chain (sel -> meta -> jumps) leaves together with the loads of
  // the staging, so that the round trips overlap (fused phase: profiles/head_batch_static.txt shows
  // what the compiler makes of it; the separate kernels keep the plain form)
  uint32_t selL = 0, selM = 0, selR = 0;
  // FUSED: the buffers of the columns two sites away, for the acceptance stage's outer triples (they
  // belong to other colours and do not change in this phase), in the same batch of loads
  uint32_t selLL = 0, selRR = 0;
  const bool hasLL = FUSED && valid && S.g0 + site > 1u, hasRR = FUSED && valid && S.g0 + site < S.n_global - 2u;
  if constexpr (FUSED) {
    // ONE batch of loads, one wait: everything whose address is known at entry.  A load under a
    // condition compiles to a branch and a wait of its own, so every load here is unconditional,
    // its address clamped to one that is always in range (`first` is a site of this launch), and
    // the condition selects the value afterwards.  This lane's share of the matrix table and of the
    // constants waits in registers; the LDS writes follow the batch.
    constexpr int TK = SMALL ? (NBA * 4 * (int)EPV_SEGTAB_DBL + 63) / 64 : 6;   // table doubles per lane (generic: B <= 16 at 64 lanes)
    const uint8_t *psel = S.sel + (valid ? site : first);
    const uint32_t rL = psel[-1], rM = psel[0], rR = psel[1];
    const uint32_t rLL = *(hasLL ? psel - 2 : psel), rRR = *(hasRR ? psel + 2 : psel);
    double r_tab[TK];
#pragma unroll
    for (int k = 0; k < TK; ++k) {
      const uint32_t i = threadIdx.x + (uint32_t)k * blockDim.x;
      r_tab[k] = segtab[i < tab_dbl ? i : 0u];
    }
    const uint32_t ci = threadIdx.x < 20u + NNODE ? threadIdx.x : 0u;
    const double *cbase = ci < 20u ? reinterpret_cast<const double *>(S.model) : S.blen;
    const double r_c = cbase[ci < 20u ? ci : ci - 20u];
    // (the writes are unconditional too -- under a condition the compiler sinks the load into the
    // branch and waits there: a lane beyond the end writes entry 0 with entry 0's value once more)
#pragma unroll
    for (int k = 0; k < TK; ++k) {
      const uint32_t i = threadIdx.x + (uint32_t)k * blockDim.x;
      s_tab[i < tab_dbl ? i : 0u] = r_tab[k];
    }
    s_const[ci] = r_c;
    if constexpr (!SMALL) {     // (a tree beyond the registers' share: the rest as stage_constants does it)
      for (uint32_t i = threadIdx.x + (uint32_t)TK * blockDim.x; i < tab_dbl; i += blockDim.x) s_tab[i] = segtab[i];
      for (uint32_t i = threadIdx.x + blockDim.x; i < 20u + NNODE; i += blockDim.x) s_const[i] = S.blen[i - 20u];
    }
    __syncthreads();
    selL = valid ? rL : 0u; selM = valid ? rM : 0u; selR = valid ? rR : 0u;
    selLL = hasLL ? rLL : 0u; selRR = hasRR ? rRR : 0u;
  } else {
    if (valid) { selL = S.sel[site - 1]; selM = S.sel[site]; selR = S.sel[site + 1]; }
    for (uint32_t i = threadIdx.x; i < tab_dbl; i += blockDim.x) s_tab[i] = segtab[i];
    stage_constants(S, s_const);
  }
  const double *s_rates = s_const;
  const double *s_blen = s_const + 20;

  // plane offsets without per-lane 64-bit multiplies (quarter-rate on the vector unit): the buffer
  // select is a conditional add, the branch stride a wave-uniform product
  const uint64_t Bn = (uint64_t)B * n, Cn = (uint64_t)S.C * n;
  const uint64_t mbaseL = (selL ? Bn : 0ull) + (site - 1), mbaseR = (selR ? Bn : 0ull) + (site + 1);
  const uint64_t mbaseM = (selM ? Bn : 0ull) + site;
  const uint64_t jbaseL = (selL ? Bn * S.C : 0ull) + (site - 1), jbaseR = (selR ? Bn * S.C : 0ull) + (site + 1);
  uint32_t need_rec = 0, heavy = 0;
  // SMALL: the topology in ONE scalar register (bit node: a leaf; bits 8 + 3 node ..: the parent); per branch ONE register of what this lane's own passes
  // read: this site's meta word (bits 0..15), the segment count K <= 2C + 1 <= 64 (bits 16..23) and
  // the start states of the left / right neighbour (bits 25 / 24: the matrix table's column)
  uint32_t topo = 0u, r_w[NBA];
#define EPV_TOPO_LEAF(node) ((topo >> (node)) & 1u)
#define EPV_TOPO_PARENT(node) ((topo >> (8 + 3 * (node))) & 7u)
#define EPV_RW_META(w) ((w) & 0xffffu)
#define EPV_RW_K(w) (((w) >> 16) & 0xffu)
#define EPV_RW_TAB(w) ((w) >> 24)
  if constexpr (SMALL) {
    topo = F.topo;     // (the host packs it: a kernel argument, no load)
#pragma unroll
    for (int b = 0; b < NN - 1; ++b) r_w[b] = 1u << 16;
  }
  // FUSED: the two outer columns no neighbour lane holds (s_edge) travel in the batch of the meta
  // words: lane 0 fetches the column two sites to its left, the last valid lane the one two sites
  // to its right (one lane may be both), zero where the genome ends.  No condition on loads or
  // writes here either: every lane loads two words per branch and writes them, a lane without that
  // outer column its own site's word once more, into the slot that word has anyway.
  const unsigned long long vmask = __ballot(valid);
  const int last_lane = vmask ? 63 - __clzll((long long)vmask) : 0;
  const bool edgeL = lane == 0, edgeR = lane == last_lane;
  const uint64_t ebaseL = edgeL && hasLL ? (selLL ? Bn : 0ull) + (site - 2) : mbaseM;
  const uint64_t ebaseR = edgeR && hasRR ? (selRR ? Bn : 0ull) + (site + 2) : mbaseM;
  // slot of branch b in s_meta: at + b * step (s_edge = s_meta + 3 B 64)
  const uint32_t own_at = 2u * B * 64u + (uint32_t)lane;
  const uint32_t eatL = edgeL ? 3u * B * 64u : own_at, estepL = edgeL ? 1u : 64u;
  const uint32_t eatR = edgeR ? 3u * B * 64u + B : own_at, estepR = edgeR ? 1u : 64u;
  const bool ezeroL = edgeL && !hasLL, ezeroR = edgeR && !hasRR;
  if (SMALL && valid) {
    uint32_t mL[NBA], mR[NBA], mM[NBA], eL[NBA], eR[NBA];
#pragma unroll
    for (int b = 0; b < NBA; ++b) {
      mL[b] = S.meta[mbaseL + (uint64_t)b * n];
      mR[b] = S.meta[mbaseR + (uint64_t)b * n];
      mM[b] = S.meta[mbaseM + (uint64_t)b * n];
      eL[b] = S.meta[ebaseL + (uint64_t)b * n];
      eR[b] = S.meta[ebaseR + (uint64_t)b * n];
    }
#pragma unroll
    for (int b = 0; b < NBA; ++b) {
      s_meta[eatL + (uint32_t)b * estepL] = ezeroL ? (epv_meta_t)0 : (epv_meta_t)eL[b];
      s_meta[eatR + (uint32_t)b * estepR] = ezeroR ? (epv_meta_t)0 : (epv_meta_t)eR[b];
    }
#pragma unroll
    for (int b = 0; b < NBA; ++b) {
      s_meta[(0u * B + b) * 64u + lane] = (epv_meta_t)mL[b];
      s_meta[(1u * B + b) * 64u + lane] = (epv_meta_t)mR[b];
      s_meta[(2u * B + b) * 64u + lane] = (epv_meta_t)mM[b];
      const uint32_t K = (mL[b] & EPV_NJ_MASK) + (mR[b] & EPV_NJ_MASK) + 1u;
      r_w[b] = (uint32_t)(epv_meta_t)mM[b] | (K << 16) | ((2u * (mL[b] >> EPV_INIT_SHIFT) + (mR[b] >> EPV_INIT_SHIFT)) << 24);
      need_rec += K + (!LEAF && EPV_TOPO_LEAF(b + 1) ? 0u : 1u);
      if (K >= 2u) heavy += K;
    }
  } else if (!SMALL && valid) {
#pragma unroll 4
    for (uint32_t b = 0; b < B; ++b) {
      const uint32_t mL = S.meta[mbaseL + (uint64_t)b * n];
      const uint32_t mR = S.meta[mbaseR + (uint64_t)b * n];
      const uint32_t mM = S.meta[mbaseM + (uint64_t)b * n];
      if constexpr (FUSED) {
        const uint32_t eL = S.meta[ebaseL + (uint64_t)b * n];
        const uint32_t eR = S.meta[ebaseR + (uint64_t)b * n];
        s_meta[eatL + b * estepL] = ezeroL ? (epv_meta_t)0 : (epv_meta_t)eL;
        s_meta[eatR + b * estepR] = ezeroR ? (epv_meta_t)0 : (epv_meta_t)eR;
      }
      s_meta[(0u * B + b) * 64u + lane] = (epv_meta_t)mL;
      s_meta[(1u * B + b) * 64u + lane] = (epv_meta_t)mR;
      s_meta[(2u * B + b) * 64u + lane] = (epv_meta_t)mM;
      const uint32_t K = (mL & EPV_NJ_MASK) + (mR & EPV_NJ_MASK) + 1u;
      need_rec += K + (LEAF || S.subtree[b + 1u] != 1u ? 1u : 0u);
      if (K >= 2u) heavy += K;
    }
  }
  P2_MARK(0);
  // FUSED: lengths of the wave's private lists (wave-uniform), and which lanes' sites await acceptance
  uint32_t f_nseg = 0u, f_nbt = 0u, f_nsole = 0u;    // f_nsole: branches with one dirty segment
  bool f_listed = false;
  const uint64_t f_wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave_id;
  bool pending = valid;
  // SMALL: this lane's row of the node table (the generic body's regA[node][lane])
  uint32_t r_node[NNA];
#pragma unroll
  for (int node = 0; node < NNA; ++node) r_node[node] = 0u;
  while (__any(pending)) {
    const uint32_t wantR = pending ? need_rec : 0u, wantH = pending ? heavy : 0u;
    const uint32_t inclR = wave_incl_scan_u32(wantR), inclH = wave_incl_scan_u32(wantH);
    // non-decreasing in the lane index, so the lanes that run are a prefix of the pending ones
    const bool run = pending && 2u * inclR + HREC * inclH <= pool_dbl;
    const unsigned long long rmask = __ballot(run);
    const int hi_lane = rmask ? 63 - __clzll((long long)rmask) : 0;
    const uint32_t totR = rmask ? epv_bcast(inclR, hi_lane) : 0u, totH = rmask ? epv_bcast(inclH, hi_lane) : 0u;
    constexpr size_t RS = 2u;   // doubles between consecutive records of a lane
    double *my = pool + (size_t)(inclR - wantR) * 2u;
    double *list = pool + (size_t)totR * 2u;
    const uint32_t hbase = inclH - wantH;

    P2_MARK(1);
    // ---- 1. list the heavy segments: forward merge of the neighbours' jumps (Segment.cpp:35-79).
    //      The merges of different branches are independent, and a lane has a heavy branch at
    //      about every eighth (lane, node) pair of a short tree: walking the nodes with whichever
    //      lanes are heavy there kept an eighth of the wave busy.  So the heavy (lane, node)
    //      pairs are listed first (in the node table, which pruning fills only afterwards) and
    //      then merged one pair per LANE.
    auto merge_branch = [&](uint32_t owner, uint32_t node, uint32_t hcur, uint64_t jl, uint64_t jr) __attribute__((always_inline)) {
      const uint32_t b = node - 1u;
      const uint32_t cL = s_meta[(0u * B + b) * 64u + owner], cR = s_meta[(1u * B + b) * 64u + owner];
      const uint32_t K = (cL & EPV_NJ_MASK) + (cR & EPV_NJ_MASK) + 1u;
      PathRef L, R;
      L.j = S.jumps + jl + (uint64_t)b * Cn; L.nj = cL & EPV_NJ_MASK; L.init = cL >> EPV_INIT_SHIFT;
      R.j = S.jumps + jr + (uint64_t)b * Cn; R.nj = cR & EPV_NJ_MASK; R.init = cR >> EPV_INIT_SHIFT;
      uint32_t trip0 = 4u * L.init + R.init, i = 0, j = 0;
      double seg_start = 0.0;
      double tl = L.nj ? L.j[0] : EPV_INF, tr = R.nj ? R.j[0] : EPV_INF;
      for (uint32_t k = 0; k < K; ++k) {
        const bool last_seg = (k + 1u == K);
        const bool take_left = tl < tr;
        const double seg_end = last_seg ? s_blen[node] : (take_left ? tl : tr);
        double *rec = list + (size_t)(hcur + k) * HREC;
        rec[LEN_AT] = seg_end - seg_start;
        rec[INFO_AT] = epv_u2d((uint64_t)trip0 | ((uint64_t)owner << 3) | ((uint64_t)node << 9) | ((uint64_t)k << 21));
        if (!last_seg) {
          if (take_left) { trip0 ^= 4u; ++i; tl = i < L.nj ? L.j[(uint64_t)i * n] : EPV_INF; }
          else { trip0 ^= 1u; ++j; tr = j < R.nj ? R.j[(uint64_t)j * n] : EPV_INF; }
          seg_start = seg_end;
        }
      }
    };
    if (B > 1u) {      // (a single branch: every lane is its own pair)
      // 1a. pair words lane | node << 6 | first record << 18 (an LDS pool holds fewer than 2^14 records)
      uint32_t n_pairs = 0u;
      if constexpr (SMALL) {
        if (run && heavy)
#pragma unroll
          for (int b = 0; b < NBA; ++b) n_pairs += EPV_RW_K(r_w[b]) >= 2u ? 1u : 0u;   // (a jump on either side)
      } else if (run && heavy)
        for (uint32_t b = 0; b < B; ++b)
          n_pairs += ((s_meta[(0u * B + b) * 64u + lane] | s_meta[(1u * B + b) * 64u + lane]) & EPV_NJ_MASK) ? 1u : 0u;
      const uint32_t inclP = wave_incl_scan_u32(n_pairs);
      const uint32_t totP = epv_bcast(inclP, 63);
      if (SMALL && n_pairs) {
        uint32_t hcur = hbase, at = inclP - n_pairs;
#pragma unroll
        for (int node = 1; node < NNA; ++node) {
          const uint32_t K = EPV_RW_K(r_w[node - 1]);
          if (K >= 2u) { regA[at++] = (uint32_t)lane | ((uint32_t)node << 6) | (hcur << 18); hcur += K; }
        }
      } else if (n_pairs) {
        uint32_t hcur = hbase, at = inclP - n_pairs;
        for (uint32_t node = 1u; node < NNODE; ++node) {
          const uint32_t b = node - 1u;
          const uint32_t K = (s_meta[(0u * B + b) * 64u + lane] & EPV_NJ_MASK) + (s_meta[(1u * B + b) * 64u + lane] & EPV_NJ_MASK) + 1u;
          if (K < 2u) continue;
          regA[at++] = (uint32_t)lane | (node << 6) | (hcur << 18);
          hcur += K;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      // 1b. one pair per lane
      for (uint32_t p0 = 0; p0 < totP; p0 += 64u) {
        const uint32_t pidx = p0 + (uint32_t)lane;
        const uint32_t pr = pidx < totP ? regA[pidx] : 0u;
        const uint32_t owner = pr & 63u;
        const uint64_t jl = (uint64_t)__shfl((uint32_t)jbaseL, (int)owner) | ((uint64_t)__shfl((uint32_t)(jbaseL >> 32), (int)owner) << 32);
        const uint64_t jr = (uint64_t)__shfl((uint32_t)jbaseR, (int)owner) | ((uint64_t)__shfl((uint32_t)(jbaseR >> 32), (int)owner) << 32);
        if (pidx < totP) merge_branch(owner, (pr >> 6) & 4095u, pr >> 18, jl, jr);
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();     // regA goes back to pruning
    } else if (run && heavy) {
      uint32_t hcur = hbase;
      for (uint32_t node = 1u; node < NNODE; ++node) {
        const uint32_t b = node - 1u;
        const uint32_t K = (s_meta[(0u * B + b) * 64u + lane] & EPV_NJ_MASK) + (s_meta[(1u * B + b) * 64u + lane] & EPV_NJ_MASK) + 1u;
        if (K < 2u) continue;
        merge_branch((uint32_t)lane, node, hcur, jbaseL, jbaseR);
        hcur += K;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();

    P2_MARK(2);
    // ---- 2. evaluate them densely, one segment per lane (FUSED: pass 1 of two, what pruning reads)
    for (uint32_t i = (uint32_t)lane; i < totH; i += 64u) {
      double *rec = list + (size_t)i * HREC;
      const double len = rec[LEN_AT];
      const uint64_t info = epv_d2u(rec[INFO_AT]);
      const uint32_t trip0 = (uint32_t)info & 7u, owner = (uint32_t)(info >> 3) & 63u;
      const uint32_t node = (uint32_t)(info >> 9) & 4095u, k = (uint32_t)(info >> 21);
      if constexpr (FUSED) {
        double m[2];
        epv_seg_prune_matrix(len, s_rates[trip0], s_rates[trip0 | 2u], m);
        rec[0] = m[0];
        rec[1] = m[1];
      } else {
        double m[6];
        epv_seg_matrices(len, s_rates[trip0], s_rates[trip0 | 2u], m);
        const epv_block2 blk = epv_keyed_block<!FUSED>(seed_lo, seed_hi, gsite_lane0 + 3u * owner, sweep, node, k, 0u, 0u);
#pragma unroll
        for (int q = 0; q < 6; ++q) rec[q] = m[q];
        rec[6] = blk.d0;
        rec[7] = blk.d1;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();

    P2_MARK(3);
    bool ident = true;
    if (run) {
      // ---- 3. pruning, reverse pre-order (SingleSiteSampler.cpp:116-157)
      uint32_t off = need_rec, hcur = hbase + heavy;
      // (small tree: kept rolled -- unrolled, the scheduler hoisted every node's loads and the kernel
      // spilled to scratch from NN = 3 on)
#pragma unroll 1
      for (uint32_t node = NNODE - 1u; node >= 1u; --node) {
        const uint32_t b = node - 1u;
        // LEAF: the cell's word leaves first (its address is node and site), the LDS reads below behind it
        [[maybe_unused]] uint32_t leaf_word = 0u;
        if constexpr (LEAF) {
          if (SMALL ? EPV_TOPO_LEAF(node) != 0u : S.subtree[node] == 1u) leaf_word = epv_leaf_word(LS, node, site);
        }
        const uint32_t mL = s_meta[(0u * B + b) * 64u + lane], mR = s_meta[(1u * B + b) * 64u + lane];
        const uint32_t K = (mL & EPV_NJ_MASK) + (mR & EPV_NJ_MASK) + 1u;
        // SMALL: the tree's shape from the topology word -- no load on the chain.  (S.subtree[] is
        // wave-uniform, yet the compiler fetched it with a vector load and a full wait per node and child.)
        const uint32_t sub = SMALL ? 2u - EPV_TOPO_LEAF(node) : S.subtree[node];     // (SMALL: 1 = a leaf, that is all it says)
        off -= K + (LEAF || sub != 1u ? 1u : 0u);
        double n0 = 1.0, n1 = 1.0;
        if (sub == 1u) {
          const uint32_t mM = s_meta[(2u * B + b) * 64u + lane];
          const uint32_t leaf_state = (mM >> EPV_INIT_SHIFT) ^ (mM & 1u);
          n0 = leaf_state ? 0.0 : 1.0;
          n1 = leaf_state ? 1.0 : 0.0;
          if constexpr (LEAF) {
            epv_leaf_q(leaf_word, leaf_state, n0, n1);
            double *recq = my + (size_t)(off + K) * RS;
            recq[0] = n0; recq[1] = n1;
          }
        } else {
          if constexpr (SMALL) {
            // the children are the later nodes whose parent this is, in ascending order: the order of
            // the stride walk below, so the products take their factors in the same order
            for (uint32_t c = node + 1u; c < NNODE; ++c) {
              if (EPV_TOPO_PARENT(c) != node) continue;
              const double *a = my + (size_t)(regA[c * 64u + lane] & 0x3fffffffu) * RS;
              n0 *= a[0];
              n1 *= a[1];
            }
          } else
          for (uint32_t ch = 1u; ch < sub; ch += S.subtree[node + ch]) {
            const double *a = my + (size_t)(regA[(node + ch) * 64u + lane] & 0x3fffffffu) * RS;
            n0 *= a[0];   // p.front() of the child's branch
            n1 *= a[1];
          }
          double *recq = my + (size_t)(off + K) * RS;
          recq[0] = n0; recq[1] = n1;
        }
        regA[node * 64u + lane] = off;
        if (K == 1u) {
          const double *t = s_tab + (b * 4u + 2u * (mL >> EPV_INIT_SHIFT) + (mR >> EPV_INIT_SHIFT)) * EPV_SEGTAB_DBL;   // (32-bit index: an LDS address)
          const double P00 = t[0], P11 = t[1];
          const double P01 = 1.0 - P00, P10 = 1.0 - P11;
          double *rec = my + (size_t)off * RS;
          rec[0] = P00 * n0 + P01 * n1;
          rec[1] = P10 * n0 + P11 * n1;
        } else {
          hcur -= K;
          for (uint32_t kk = K; kk-- > 0u;) {
            const double *hr = list + (size_t)(hcur + kk) * HREC;
            const double P00 = hr[0], P11 = hr[1];
            const double P01 = 1.0 - P00, P10 = 1.0 - P11;
            const double a = P00 * n0 + P01 * n1;
            const double c = P10 * n0 + P11 * n1;
            double *rec = my + (size_t)(off + kk) * RS;
            rec[0] = a; rec[1] = c;
            n0 = a; n1 = c;
          }
        }
      }
    }

    P2_MARK(4);
    if constexpr (FUSED) {
      // ---- 3b. dense evaluation, pass 2: pruning has read P00 and P11 for the last time; the downward pass's
      //      fields -- PT00, PT10, the no-jump bounds and the segment's Philox block -- take slots 0..5
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      for (uint32_t i = (uint32_t)lane; i < totH; i += 64u) {
        double *rec = list + (size_t)i * HREC;
        const double len = rec[LEN_AT];
        const uint64_t info = epv_d2u(rec[INFO_AT]);
        const uint32_t trip0 = (uint32_t)info & 7u, owner = (uint32_t)(info >> 3) & 63u;
        const uint32_t node = (uint32_t)(info >> 9) & 4095u, k = (uint32_t)(info >> 21);
        double m[4];
        epv_seg_sample_matrices(len, s_rates[trip0], s_rates[trip0 | 2u], m);
        const epv_block2 blk = epv_keyed_block<!FUSED>(seed_lo, seed_hi, gsite_lane0 + 3u * owner, sweep, node, k, 0u, 0u);
        rec[F_PT] = m[0];
        rec[F_PT + 1u] = m[1];
        rec[F_NB] = m[2];
        rec[F_NB + 1u] = m[3];
        rec[F_UEND] = blk.d0;
        rec[F_UFIRST] = blk.d1;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      P2_MARK(10);
    }
    // ---- 4. downward sampling of the segment END STATES (:180-255); the jump times are drawn
    //         by epv_mh_jumps_kernel for the dirty branches only (see epv_kernels.h).  The node
    //         loop is wave-uniform: the task flush inside it is a wave-wide operation.
    unsigned long long dirty = 0ull, multi = 0ull, deep = 0ull;
    const uint32_t root_state = run ? (uint32_t)(s_meta[(2u * B) * 64u + lane] >> EPV_INIT_SHIFT) : 0u;
    uint32_t hcur = hbase;
    if constexpr (SMALL) {
      // (small tree: the fused phase's dense emission; nothing in this loop is wave-wide)
      if (run) {
        // the node table's row of this lane, one batch of independent LDS reads
#pragma unroll
        for (int node = 1; node < NNA; ++node) r_node[node] = regA[(uint32_t)node * 64u + lane];
#pragma unroll
        for (int node = 1; node < NNA; ++node) {
          const int b = node - 1;
          const uint32_t K = EPV_RW_K(r_w[b]);
          const uint32_t off = r_node[node];
          uint32_t start_state = root_state;
#pragma unroll
          for (int p = 1; p < node; ++p)
            if (EPV_TOPO_PARENT(node) == (uint32_t)p) start_state = r_node[p] >> 31;
          const bool leaf = EPV_TOPO_LEAF(node);
          const uint32_t mM = EPV_RW_META(r_w[b]);
          uint32_t prev = start_state;
          bool clean = true;
          unsigned long long word = 0ull, w64 = 0ull, dmask = 0ull;
          double pk0 = my[(size_t)off * RS], pk1 = my[(size_t)off * RS + 1u];
          for (uint32_t k = 0; k < K; ++k) {
            const bool last_seg = (k + 1u == K);
            double nxt0, nxt1;
            if (!LEAF && last_seg && leaf) {          // q of a leaf: the observed state (LEAF: the record pruning filed)
              const uint32_t leaf_state = (mM >> EPV_INIT_SHIFT) ^ (mM & 1u);
              nxt0 = leaf_state ? 0.0 : 1.0;
              nxt1 = leaf_state ? 1.0 : 0.0;
            } else {
              nxt0 = my[(size_t)(off + k + 1u) * RS];      // p[k+1], or the node's q
              nxt1 = my[(size_t)(off + k + 1u) * RS + 1u];
            }
            double PT0, nb, u_end, u_first;
            if (K == 1u) {
              const double *t = s_tab + ((uint32_t)b * 4u + EPV_RW_TAB(r_w[b])) * EPV_SEGTAB_DBL;
              PT0 = prev ? t[3] : t[2];
              nb = prev ? t[5] : t[4];
              const epv_block2 blk = epv_keyed_block<!FUSED>(seed_lo, seed_hi, gsite, sweep, (uint32_t)node, 0u, 0u, 0u);
              u_end = blk.d0; u_first = blk.d1;
            } else {
              const double *hr = list + (size_t)(hcur + k) * HREC;
              PT0 = prev ? hr[F_PT + 1u] : hr[F_PT];
              nb = prev ? hr[F_NB + 1u] : hr[F_NB];
              u_end = hr[F_UEND]; u_first = hr[F_UFIRST];
            }
            const double p0 = PT0 * nxt0 / (prev ? pk1 : pk0);
            const uint32_t sampled = (u_end > p0) ? 1u : 0u;
            const bool seg_clean = (sampled == prev) && (1.0 - u_first < nb);
            clean = clean && seg_clean;
            if (!seg_clean) dmask |= 1ull << (k & 63u);
            word |= (unsigned long long)sampled << (k & 63u);
            if (k < 64u) w64 = word;
            prev = sampled;
            pk0 = nxt0; pk1 = nxt1;
          }
          const uint32_t hrec0 = hcur;
          if (K >= 2u) hcur += K;
          // node table row for the children and the emission pass (see the generic body below); the
          // emission pass reads other lanes' rows, so the row goes to LDS as well
          r_node[node] = off | (prev << 31) | (clean ? 0u : 1u << 30) | (K >= 2u ? hrec0 << 14 : 0u);
          regA[node * 64u + lane] = r_node[node];
          if (!clean && K >= 2u) {
            list[(size_t)hrec0 * HREC + F_W64] = epv_u2d(w64);
            list[(size_t)hrec0 * HREC + F_DMASK] = epv_u2d(dmask);
          }
          s_meta[(2u * B + (uint32_t)b) * 64u + lane] = (epv_meta_t)(start_state << EPV_INIT_SHIFT);
          ident = ident && clean && mM == (start_state << EPV_INIT_SHIFT);
        }
      }
    } else
    for (uint32_t node = 1u; node < S.N; ++node) {
      const uint32_t b = node - 1u;
      // what the wave-wide hand-over below needs from this lane's branch
      uint32_t nds = 0, Kb = 0, st_b = 0, end_b = 0, hrec0 = 0, trip_b = 0;
      unsigned long long w64 = 0ull, dmask = 0ull;     // (dmask, FUSED: the branch's dirty segments, for the hand-over)
      bool dirty_b = false;
      if (run) {
        const uint32_t mL = s_meta[(0u * B + b) * 64u + lane], mR = s_meta[(1u * B + b) * 64u + lane];
        const uint32_t K = (mL & EPV_NJ_MASK) + (mR & EPV_NJ_MASK) + 1u;
        const uint32_t off = regA[node * 64u + lane];
        const uint32_t par = S.parent[node];
        const uint32_t start_state = (par == 0u) ? root_state : (regA[par * 64u + lane] >> 31);
        const bool leaf = S.subtree[node] == 1u;
        const uint32_t mM = s_meta[(2u * B + b) * 64u + lane];
        uint32_t prev = start_state;
        bool clean = true;
        unsigned long long word = 0ull;
        uint64_t *states = S.prop_states + ((uint64_t)b * S.phase_cap + tid) * S.W;
        double pk0 = my[(size_t)off * RS], pk1 = my[(size_t)off * RS + 1u];
        for (uint32_t k = 0; k < K; ++k) {
          const bool last_seg = (k + 1u == K);
          double nxt0, nxt1;
          if (!LEAF && last_seg && leaf) {          // q of a leaf: the observed state (LEAF: the record pruning filed)
            const uint32_t leaf_state = (mM >> EPV_INIT_SHIFT) ^ (mM & 1u);
            nxt0 = leaf_state ? 0.0 : 1.0;
            nxt1 = leaf_state ? 1.0 : 0.0;
          } else {
            nxt0 = my[(size_t)(off + k + 1u) * RS];      // p[k+1], or the node's q
            nxt1 = my[(size_t)(off + k + 1u) * RS + 1u];
          }
          double PT0, nb, u_end, u_first;
          if (K == 1u) {
            const double *t = s_tab + (b * 4u + 2u * (mL >> EPV_INIT_SHIFT) + (mR >> EPV_INIT_SHIFT)) * EPV_SEGTAB_DBL;   // (32-bit index: an LDS address)
            PT0 = prev ? t[3] : t[2];
            nb = prev ? t[5] : t[4];
            const epv_block2 blk = epv_keyed_block<!FUSED>(seed_lo, seed_hi, gsite, sweep, node, 0u, 0u, 0u);
            u_end = blk.d0; u_first = blk.d1;
          } else {
            const double *hr = list + (size_t)(hcur + k) * HREC;
            PT0 = prev ? hr[F_PT + 1u] : hr[F_PT];
            nb = prev ? hr[F_NB + 1u] : hr[F_NB];
            u_end = hr[F_UEND]; u_first = hr[F_UFIRST];
          }
          const double p0 = PT0 * nxt0 / (prev ? pk1 : pk0);
          const uint32_t sampled = (u_end > p0) ? 1u : 0u;
          // trial 1's first draw is the other half of the same Philox block: a segment that keeps
          // its state and provably has no jump in trial 1 is clean
          const bool seg_clean = (sampled == prev) && (1.0 - u_first < nb);
          clean = clean && seg_clean;
          nds += seg_clean ? 0u : 1u;
          if (FUSED && !seg_clean) dmask |= 1ull << (k & 63u);
          word |= (unsigned long long)sampled << (k & 63u);
          if (k < 64u) w64 = word;
          if (!FUSED && (k & 63u) == 63u) { states[k >> 6] = word; word = 0ull; }   // (the fused phase hands the states over in its segment tasks)
          prev = sampled;
          pk0 = nxt0; pk1 = nxt1;
        }
        hrec0 = hcur;
        if (K >= 2u) hcur += K;
        if (!FUSED && (K & 63u) && !clean) states[(K - 1u) >> 6] = word;   // only a dirty branch is read back
        // FUSED: proposal end state for the children (bit 31); "dirty" (bit 30) and the branch's first
        // heavy record (bits 14..27) for the emission pass behind this loop, which gives every dirty
        // (site, branch) pair its own lane; the sampled end states of a heavy branch wait in the
        // slot of its first record's end-state uniform, which has been used
        if (FUSED) {
          regA[node * 64u + lane] = off | (prev << 31) | (clean ? 0u : 1u << 30) | (K >= 2u ? hrec0 << 14 : 0u);
          if (!clean && K >= 2u) {
            list[(size_t)hrec0 * HREC + F_W64] = epv_u2d(w64);
            list[(size_t)hrec0 * HREC + F_DMASK] = epv_u2d(dmask);
          }
        } else
          regA[node * 64u + lane] = off | (prev << 31);  // proposal end state for the children
        // the proposal's meta word (start state, no jumps yet; the fused phase's assembly adds the
        // count) takes the place of the current path's, which this lane has just read for the last
        // time: the acceptance stage finds it there.  (NOT in the node table: a later round of this
        // wave lists its heavy pairs over the finished lanes' rows.)
        if (FUSED) s_meta[(2u * B + b) * 64u + lane] = (epv_meta_t)(start_state << EPV_INIT_SHIFT);
        // same as the current path?  (no jumps on either, same start state)
        ident = ident && clean && mM == (start_state << EPV_INIT_SHIFT);
        dirty_b = !clean;
        Kb = K; st_b = start_state; end_b = prev;
        trip_b = 4u * (mL >> EPV_INIT_SHIFT) + (mR >> EPV_INIT_SHIFT);
      }
      bool old_list = dirty_b;
      if (SEG && !FUSED) {
        // ---- dirty SEGMENTS onto the segment list (one lane each in epv_seg_search_kernel) and the
        //      branch onto the assemble list: one atomic per wave and node reserves both ranges.
        //      A branch with more than 64 segments, or one that finds the lists full, takes the
        //      bucketed lists of the sequential kernel instead.
        const bool cand = dirty_b && Kb <= 64u;
        const uint32_t wS = cand ? nds : 0u, wB = cand ? 1u : 0u;
        const uint32_t inclS = wave_incl_scan_u32(wS), inclB = wave_incl_scan_u32(wB);
        const uint32_t totS = epv_bcast(inclS, 63), totB = epv_bcast(inclB, 63);
        if (totB) {
          const uint32_t shard = my_shard;
          uint32_t bS, bB;
          if (FUSED) {
            bS = f_nseg; bB = f_nbt;
            f_nseg += totS; f_nbt += totB;
          } else {
            unsigned long long base = 0ull;
            if (lane == 0)
              base = atomicAdd(&counters[EPV_CNT_IDX(EPV_CNT_SEG, shard)],
                               (unsigned long long)totS | ((unsigned long long)totB << 32));
            bS = epv_bcast((uint32_t)base, 0); bB = epv_bcast((uint32_t)(base >> 32), 0);
          }
          if (cand) {
            const uint64_t i0 = (uint64_t)bS + (inclS - wS), j0 = (uint64_t)bB + (inclB - 1u);
            EpvSegTask *segs = FUSED ? F.segs + f_wave * F.seg_cap : S.segs + (uint64_t)shard * S.seg_cap;
            unsigned long long *btl = FUSED ? F.bt + f_wave * F.bt_cap : S.btasks + (uint64_t)shard * S.btask_cap;
            uint32_t *bfl = FUSED ? F.bfirst + f_wave * F.bt_cap : S.bfirst + (uint64_t)shard * S.btask_cap;
            const uint64_t seg_room = FUSED ? F.seg_cap : S.seg_cap, bt_room = FUSED ? F.bt_cap : S.btask_cap;
            if (i0 + nds <= seg_room && j0 < bt_room) {
              btl[j0] = site | ((unsigned long long)b << 40) | ((unsigned long long)nds << 52) | ((unsigned long long)end_b << 59) |
                        ((unsigned long long)st_b << 60) | ((unsigned long long)(selM ^ 1u) << 61);
              bfl[j0] = (uint32_t)i0;
              uint32_t prev = st_b;
              double tp = 0.0;     // running sum of the segment lengths (SingleSiteSampler.cpp:218)
              uint64_t at = i0;
              for (uint32_t k = 0; k < Kb; ++k) {
                const uint32_t sampled = (uint32_t)(w64 >> k) & 1u;
                double len;
                uint32_t trip0;
                bool seg_clean;
                if (Kb == 1u) {
                  len = s_blen[node];
                  trip0 = trip_b;
                  seg_clean = false;       // the only segment of a dirty branch
                } else {
                  const double *hr = list + (size_t)(hrec0 + k) * HREC;
                  len = hr[LEN_AT];
                  trip0 = (uint32_t)epv_d2u(hr[INFO_AT]) & 7u;
                  seg_clean = (sampled == prev) && (1.0 - hr[7] < (prev ? hr[5] : hr[4]));
                }
                if (!seg_clean) {
                  EpvSegTask t;
                  t.w0 = site | ((unsigned long long)node << 40) | ((unsigned long long)k << 52);
                  t.len = len;
                  t.start = tp;
                  t.w3 = prev | (sampled << 1) | (trip0 << 2);
                  segs[at++] = t;
                }
                tp += len;
                prev = sampled;
              }
              old_list = false;
            } else {
              // no room: blank what this lane reserved inside the lists, fall back
              for (uint64_t i = i0; i < i0 + nds && i < seg_room; ++i) segs[i].len = -1.0;
              if (j0 < bt_room) btl[j0] = ~0ull;
            }
          }
        }
      }
      if (!FUSED && old_list) {      // (the fused phase's lists hold the worst case: never taken there)
        dirty |= 1ull << (b & 63u);
        if (Kb == 2u || Kb >= 4u) multi |= 1ull << (b & 63u);   // four buckets by segment count
        if (Kb >= 3u) deep |= 1ull << (b & 63u);
      }
      if (!FUSED && ((b & 63u) == 63u || node + 1u == S.N)) {
        epv_flush_tasks(S, counters, dirty, multi, deep, b, site, lane, my_shard);
        dirty = multi = deep = 0ull;
      }
    }

    P2_MARK(5);
    // ---- 5. hand-over.  A proposal equal to the current path is accepted with probability one
    //         and changes neither the paths nor the cached likelihoods: count it and be done.
    //         Everything else: start states of the proposal's branches into the other buffer,
    //         and the site onto the accept list of this block's shard.
    const bool to_list = run && !ident;
    if (SMALL && to_list) {
#pragma unroll
      for (int node = 1; node < NNA; ++node) {
        uint32_t st = root_state;
#pragma unroll
        for (int p = 1; p < node; ++p)
          if (EPV_TOPO_PARENT(node) == (uint32_t)p) st = r_node[p] >> 31;
        S.meta[(selM ? 0ull : Bn) + (uint64_t)(node - 1) * n + site] = (epv_meta_t)(st << EPV_INIT_SHIFT);
      }
      // (the overflow flag of a small-tree body stays in the wave: cleared behind the rounds, below)
    } else if (!SMALL && to_list) {
      for (uint32_t node = 1u; node < S.N; ++node) {
        const uint32_t par = S.parent[node];
        const uint32_t st = (par == 0u) ? root_state : (regA[par * 64u + lane] >> 31);
        S.meta[(selM ? 0ull : Bn) + (uint64_t)(node - 1u) * n + site] = (epv_meta_t)(st << EPV_INIT_SHIFT);
      }
      S.prop_flag[tid] = 0u;
    }
    {
      const uint32_t shard = my_shard;
      f_listed = f_listed || to_list;
      const unsigned long long lm = FUSED ? 0ull : __ballot(to_list);
      if (lm) {
        unsigned long long base = 0ull;
        if (lane == 0)
          base = atomicAdd(&counters[EPV_CNT_IDX(parity ? EPV_CNT_ALIST1 : EPV_CNT_ALIST0, shard)],
                           (unsigned long long)__popcll(lm));
        const uint32_t b0 = epv_bcast((uint32_t)base, 0);
        if (to_list)
          S.alist[(uint64_t)shard * S.alist_cap + b0 + (uint32_t)__popcll(lm & ((1ull << lane) - 1ull))] = (uint32_t)tid;
      }
      const unsigned long long am = __ballot(run && ident && site >= own_first && site <= own_last);
      if (am && lane == 0)
        atomicAdd(&counters[EPV_CNT_IDX(EPV_CNT_ACCEPT, shard)], (unsigned long long)__popcll(am));
    }
    if (FUSED) {
      // ---- 6. the dirty (site, branch) pairs of this round, ONE LANE EACH: their dirty segments
      //      onto the wave's segment list, the branch onto its assemble list.  (Doing this inside the
      //      node loop cost two wave scans and ~130 instructions per node for the one lane in
      //      fourteen that had a dirty branch there.)  The pair list lives in the Felsenstein records
      //      of this round, which are dead now; everything a pair needs is in the node table, the
      //      staged meta words and the heavy records.
      uint32_t *plist = reinterpret_cast<uint32_t *>(pool);
      uint32_t npair = 0u;
      if constexpr (SMALL) {
        if (run)
#pragma unroll
          for (int node = 1; node < NNA; ++node) npair += (r_node[node] >> 30) & 1u;
      } else if (run)
        for (uint32_t node = 1u; node < S.N; ++node) npair += (regA[node * 64u + lane] >> 30) & 1u;
      const uint32_t inclP = wave_incl_scan_u32(npair);
      const uint32_t totP = epv_bcast(inclP, 63);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (SMALL && npair) {
        uint32_t at = inclP - npair;
#pragma unroll
        for (int node = 1; node < NNA; ++node)
          if ((r_node[node] >> 30) & 1u) plist[at++] = (uint32_t)lane | ((uint32_t)node << 6);
      } else if (npair) {
        uint32_t at = inclP - npair;
        for (uint32_t node = 1u; node < S.N; ++node)
          if ((regA[node * 64u + lane] >> 30) & 1u) plist[at++] = (uint32_t)lane | (node << 6);
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint64_t site_lane0 = site - 3u * (uint64_t)lane;
      EpvSegTask *segs_w = F.segs + f_wave * F.seg_cap;
      unsigned long long *btl = F.bt + f_wave * F.bt_cap;
      uint32_t *bfl = F.bfirst + f_wave * F.bt_cap;
      for (uint32_t p0 = 0; p0 < totP; p0 += 64u) {
        const uint32_t pidx = p0 + (uint32_t)lane;
        const bool act = pidx < totP;
        const uint32_t pr = act ? plist[pidx] : 0u;
        const uint32_t owner = pr & 63u, node = act ? pr >> 6 : 1u, b = node - 1u;
        const uint32_t selM_o = (uint32_t)__shfl((int)selM, (int)owner);
        const uint32_t ra = regA[node * 64u + owner];
        const uint32_t end_b = ra >> 31, hrec0 = (ra >> 14) & 0x3fffu;
        const uint32_t st_b = (uint32_t)(s_meta[(2u * B + b) * 64u + owner] >> EPV_INIT_SHIFT);
        const uint32_t mL = s_meta[(0u * B + b) * 64u + owner], mR = s_meta[(1u * B + b) * 64u + owner];
        const uint32_t Kb = (mL & EPV_NJ_MASK) + (mR & EPV_NJ_MASK) + 1u;
        // which segments are dirty (trial 1 does not settle them)
        unsigned long long w64 = end_b, dmask = 1ull;
        uint32_t nds = act ? 1u : 0u;
        if (act && Kb >= 2u) {
          // (the downward pass left both in the branch's first record)
          w64 = epv_d2u(list[(size_t)hrec0 * HREC + F_W64]);
          dmask = epv_d2u(list[(size_t)hrec0 * HREC + F_DMASK]);
          nds = (uint32_t)__popcll(dmask);
        }
        const uint32_t inclS = wave_incl_scan_u32(nds);
        const uint32_t totS = epv_bcast(inclS, 63);
        if (act) {
          const uint64_t osite = site_lane0 + 3u * (uint64_t)owner;
          const uint64_t i0 = (uint64_t)f_nseg + (inclS - nds), j0 = (uint64_t)f_nbt + (uint32_t)lane;
          btl[j0] = osite | ((unsigned long long)b << 40) | ((unsigned long long)nds << 52) | ((unsigned long long)end_b << 59) |
                    ((unsigned long long)st_b << 60) | ((unsigned long long)(selM_o ^ 1u) << 61);
          bfl[j0] = (uint32_t)i0;
          uint32_t prev = st_b;
          double tp = 0.0;     // running sum of the segment lengths (SingleSiteSampler.cpp:218)
          uint64_t at = i0;
          for (uint32_t k = 0; k < Kb; ++k) {
            const uint32_t sampled = (uint32_t)(w64 >> k) & 1u;
            double len;
            uint32_t trip0;
            if (Kb == 1u) {
              len = s_blen[node];
              trip0 = 4u * (mL >> EPV_INIT_SHIFT) + (mR >> EPV_INIT_SHIFT);
            } else {
              const double *hr = list + (size_t)(hrec0 + k) * HREC;
              len = hr[LEN_AT];
              trip0 = (uint32_t)epv_d2u(hr[INFO_AT]) & 7u;
            }
            if ((dmask >> k) & 1ull) {
              EpvSegTask t;
              t.w0 = osite | ((unsigned long long)node << 40) | ((unsigned long long)k << 52);
              t.len = len;
              t.start = tp;
              // bit 5: the sole dirty segment of its branch, bit 6: the proposal's buffer -- the grouped
              // search finishes such a branch itself (epv_jumps2.h)
              t.w3 = prev | (sampled << 1) | (trip0 << 2) | (nds == 1u ? 32u | ((selM_o ^ 1u) << 6) : 0u);
              segs_w[at++] = t;
            }
            tp += len;
            prev = sampled;
          }
        }
        f_nsole += (uint32_t)__popcll(__ballot(act && nds == 1u));
        f_nseg += totS;
        f_nbt += (totP - p0 < 64u) ? totP - p0 : 64u;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();     // the pool goes to the next round's records
    }
    pending = pending && !run;
    P2_MARK(6);
  }
  if (FUSED) {
    // the pool is free now: the search's cooperative area, then the accept stage's accumulators
    // and meta cache, are carved from it (plan_p2 sizes it for both)
    const bool nielsen = !(S.flags & EPV_FLAG_FORWARD_REJECTION);
    const EpvSegTask *segs = F.segs + f_wave * F.seg_cap;
    EpvSegOut *outs = F.outs + f_wave * F.seg_cap;
    // SMALL: the sites' overflow flags, one word per lane in row 0 of the node table, which is dead
    // from here on (inside the rounds it is not: a later round lists its heavy pairs over it, so the
    // flags are cleared here and not in a round's hand-over).  The assembly raises a flag, the
    // site's owner reads it: S.prop_flag, a global round trip in front of the whole acceptance for a
    // byte the wave wrote itself, is left to the separate kernels and the generic body.
    uint32_t *s_flag = regA;
    if constexpr (SMALL) s_flag[lane] = 0u;
    // lists, start states and flags pass between the lanes of THIS wave through global memory: a
    // workgroup-scope fence (wait for the stores; one CU, one vector L1) is enough -- an agent-scope
    // one writes back and invalidates the XCD's L2, ~30 us each here
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    uint32_t f_nfin = 0u;      // branches the grouped search finished
    if constexpr (DIRECT) {
      if (f_nseg) {
        // lane l samples segments l, l + 64, ... of the wave's list at the whole capacity (the body of
        // epv_seg_search_direct_kernel); then every branch is assembled with run_direct for the replay
        for (uint32_t i = (uint32_t)lane; i < f_nseg; i += 64u)
          epv_seg_direct_one(S, s_rates, segs, outs, i, seed_lo, seed_hi, sweep, F.giveups);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        P2_MARK(7);
        for (uint32_t i = (uint32_t)lane; i < f_nbt; i += 64u)
          epv_seg_assemble_one<!FUSED, true>(S, s_rates, segs, outs, F.bt[f_wave * F.bt_cap + i], F.bfirst[f_wave * F.bt_cap + i],
                                             s0, seed_lo, seed_hi, sweep, true, s_meta + 2u * B * 64u,
                                             site - 3u * (uint64_t)lane, SMALL ? s_flag : nullptr);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        P2_MARK(8);
      }
    } else if (f_nseg) {
      EpvCoop W;
      W.len = pool; W.r0 = pool + 64; W.r1 = pool + 128; W.trunc = pool + 192; W.tj = pool + 256;
      uint32_t *u = reinterpret_cast<uint32_t *>(pool + 384);
      W.misc = u; W.gsite = u + 64; W.tbase = u + 128; W.nk = u + 192; W.res = u + 256; W.tw = u + 320; W.mm = u + 384;
      // a short list: several lanes per segment first (epv_seg_search_grouped); the wave-wide search
      // takes whatever is longer, and whatever a few rounds of that leave open
      bool done = false;
      if (f_nseg <= 32u && F.grouped_rounds) {
        const uint32_t G = 64u / f_nseg > 8u ? 8u : 64u / f_nseg;
        done = epv_seg_search_grouped<!FUSED>(S, s_rates, segs, outs, f_nseg, G, F.grouped_rounds, seed_lo, seed_hi, sweep, nielsen,
                                      s_meta + 2u * B * 64u, site - 3u * (uint64_t)lane, f_nfin);
      }
      if (!done) epv_seg_search_wave<!FUSED>(S, s_rates, W, segs, outs, f_nseg, 0u, 64u, seed_lo, seed_hi, sweep, nielsen);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
      __builtin_amdgcn_wave_barrier();
      P2_MARK(7);
      // the grouped search has finished every branch (each had one dirty segment, <= 2 jumps, room):
      // nothing is left to assemble.  In EVERY other case the assembly walks the whole branch list
      // and stores the finished branches' values once more.
      if (!(done && f_nsole == f_nbt && f_nfin == f_nbt)) {
        for (uint32_t i = (uint32_t)lane; i < f_nbt; i += 64u)
          epv_seg_assemble_one<!FUSED>(S, s_rates, segs, outs, F.bt[f_wave * F.bt_cap + i], F.bfirst[f_wave * F.bt_cap + i], s0,
                               seed_lo, seed_hi, sweep, nielsen, s_meta + 2u * B * 64u, site - 3u * (uint64_t)lane,
                               SMALL ? s_flag : nullptr);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
      P2_MARK(8);
    }
    // ---- acceptance.  A site's ratio needs the three triples around it (log_accept_rate,
    //      SingleSiteSampler.cpp:409-429); they are independent, so every (listed site, triple)
    //      pair gets its own lane -- a third of the chain, and on a short tree the lanes whose
    //      proposal equalled their path would idle anyway.  pool: own[64] | res[192] | D[8][64] |
    //      J[8][64] | meta words [3][B][64]
    bool accepted = false, overflowed = false;
    {
      uint32_t *s_own = reinterpret_cast<uint32_t *>(pool);
      double *s_res = pool + 32;
      AccLds A;
      A.d = pool + 224 + lane; A.stride = 64u;
      A.j = reinterpret_cast<uint32_t *>(pool + 736) + lane;
      epv_meta_t *mc = reinterpret_cast<epv_meta_t *>(pool + 992) + lane;
      const unsigned long long lmask = __ballot(f_listed);
      const uint32_t n_listed = (uint32_t)__popcll(lmask);
      const uint32_t my_rank = (uint32_t)__popcll(lmask & ((1ull << lane) - 1ull));
      // the owner publishes what its three task lanes need -- the five columns' buffers (known
      // since the kernel's head) and the capacity flag the assembly may have raised -- and starts
      // its own loads and its accept uniform before the tasks, whose waits then hide them
      bool ovf = false;
      double llh_l = 0.0, llh_m = 0.0, llh_r = 0.0, u_acc = 0.0;
      if (f_listed) {
        if constexpr (SMALL) ovf = s_flag[lane] != 0u;
        else ovf = S.prop_flag[tid] != 0;
        llh_l = S.tri[site - 1]; llh_m = S.tri[site]; llh_r = S.tri[site + 1];
        s_own[my_rank] = (uint32_t)lane | (selLL << 8) | (selL << 9) | ((selM ^ 1u) << 10) | (selR << 11) | (selRR << 12) |
                         ((ovf ? 1u : 0u) << 13);
        u_acc = epv_keyed_block<!FUSED>(seed_lo, seed_hi, gsite, sweep, 0u, 0u, 0u, 0u).d0;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      const uint64_t site_lane0 = site - 3u * (uint64_t)lane;
      for (uint32_t t = (uint32_t)lane; t < 3u * n_listed; t += 64u) {
        const uint32_t r = t / 3u, w = t - 3u * r, ow = s_own[r], o = ow & 63u;
        const uint64_t osite = site_lane0 + 3u * (uint64_t)o;
        const uint64_t g = S.g0 + osite;
        const bool skip = ((ow >> 13) & 1u) || (w == 0u && !(g > 1u)) || (w == 2u && !(g < S.n_global - 2u));
        double v = 0.0;
        if (!skip) {
          const uint64_t c = osite - 1u + (uint64_t)w;            // centre column of this triple
          // buffers of the three columns (bits 8.. of the owner's word: LL, L, proposal, R, RR)
          const uint32_t bl = (ow >> (8u + w)) & 1u, bm = (ow >> (9u + w)) & 1u, br = (ow >> (10u + w)) & 1u;
          if (F.meta_cache) {
            // the meta words of the triple's columns without a global round trip: the neighbours'
            // current paths were staged at the head of the kernel (they belong to other colours and
            // do not change in this phase), the proposal's sit where the site's own column was
            if constexpr (SMALL) {
              // read where they are.  A column is a row of s_meta (branch stride 64) or, for the outer
              // column of lane 0 / the last valid lane, a run of s_edge = s_meta + 3 B 64 (branch
              // stride 1): three (index, stride) pairs chosen by selects
              const uint32_t oL = 0u * B * 64u + o, oR = 1u * B * 64u + o, oP = 2u * B * 64u + o;
              const bool outL = w == 0u && o == 0u, outR = w == 2u && !(o < (uint32_t)last_lane);
              const uint32_t i0 = w == 0u ? (outL ? 3u * B * 64u : oR - 1u) : w == 1u ? oL : oP;
              const uint32_t i1 = w == 0u ? oL : w == 1u ? oP : oR;
              const uint32_t i2 = w == 0u ? oP : w == 1u ? oR : (outR ? 3u * B * 64u + B : oL + 1u);
              v = triple_llh_cached<NBA>(S, s_const, s_blen, s_meta, i0, outL ? 1u : 64u, bl, c - 1u, i1, 64u, bm, c,
                                         i2, outR ? 1u : 64u, br, c + 1u, A);
            } else {
            // (generic body: the three columns copied into the lane's private area mc first)
            const uint32_t B2 = B;
#pragma unroll 4
            for (uint32_t b = 0; b < B2; ++b) {
              const epv_meta_t mP = s_meta[(2u * B2 + b) * 64u + o];
              const epv_meta_t mL = s_meta[(0u * B2 + b) * 64u + o], mR = s_meta[(1u * B2 + b) * 64u + o];
              epv_meta_t m0, m1, m2;
              if (w == 0u) { m0 = o > 0u ? s_meta[(1u * B2 + b) * 64u + (o - 1u)] : s_edge[b]; m1 = mL; m2 = mP; }
              else if (w == 1u) { m0 = mL; m1 = mP; m2 = mR; }
              else { m0 = mP; m1 = mR; m2 = o < (uint32_t)last_lane ? s_meta[(0u * B2 + b) * 64u + (o + 1u)] : s_edge[B2 + b]; }
              mc[(0u * B2 + b) * 64u] = m0;
              mc[(1u * B2 + b) * 64u] = m1;
              mc[(2u * B2 + b) * 64u] = m2;
            }
            v = triple_llh_cached(S, s_const, s_blen, mc, 64u, 0u, bl, c - 1u, 1u, bm, c, 2u, br, c + 1u, A);
            }
          } else {
            v = triple_llh(S, s_const, s_blen, bl, c - 1u, bm, c, br, c + 1u, A);
          }
        }
        s_res[t] = v;
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      __builtin_amdgcn_wave_barrier();
      if (f_listed) {
        // the owner: Metropolis_Hastings_site :510-533 with the three values (the arithmetic of
        // epv_accept_site, term by term)
        // (no proposal ratio: the phase plan never picks this kernel when the reference's ratio or a
        // sampled root is asked for, so the term is zero by construction)
        double llr = 0.0;
        const double llh_l_orig = llh_l, llh_r_orig = llh_r;
        if (!ovf) {
          const uint64_t g = S.g0 + site;
          if (g > 1u) llh_l = s_res[3u * my_rank];
          llh_m = s_res[3u * my_rank + 1u];
          if (g < S.n_global - 2u) llh_r = s_res[3u * my_rank + 2u];
        }
        llr += (llh_l + llh_r - llh_l_orig - llh_r_orig);
        bool acc = (llr >= 0.0) || (u_acc < epv_exp(llr));
        if (ovf) { acc = false; overflowed = true; }
        if (acc) {
          S.sel[site] = (uint8_t)(selM ^ 1u);
          S.tri[site - 1] = llh_l;
          S.tri[site] = llh_m;
          S.tri[site + 1] = llh_r;
          accepted = site >= own_first && site <= own_last;
        }
      }
    }
    P2_MARK(9);
    const unsigned long long am = __ballot(accepted), om = __ballot(overflowed);
    if (lane == 0) {
      if (am) atomicAdd(&counters[EPV_CNT_IDX(EPV_CNT_ACCEPT, my_shard)], (unsigned long long)__popcll(am));
      if (om) atomicAdd(&counters[EPV_CNT_IDX(EPV_CNT_OVERFLOW, my_shard)], (unsigned long long)__popcll(om));
      if (f_nbt) atomicAdd(&counters[EPV_CNT_IDX(EPV_CNT_COOP, my_shard)], (unsigned long long)f_nbt);
      if (f_nfin) atomicAdd(&counters[EPV_CNT_IDX(EPV_CNT_SEARCH_FINISHED, my_shard)], (unsigned long long)f_nfin);
    }
  }
#ifdef EPV_P2_PROFILE
  if (epv_lane() == 0) {
    unsigned long long *row = epv_p2_prof + 16u * ((blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) % EPV_P2_PROF_ROWS);
    for (int q = 0; q < 15; ++q) row[q] += t_acc_[q];
    row[15] += 1ull;
  }
#endif
}

#endif
