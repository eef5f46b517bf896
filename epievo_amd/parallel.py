"""Site-sharded multi-GPU driver for launchers that start ONE PROCESS PER GPU (torchrun:
bench.py, the multi-process tests); the C++ EM driver shards inside one process instead
(epievo_amd/csrc/host/epv_sampler.cpp, RCCL linked directly).  Both stand on the same C-ABI
primitives and the same layout rules.

Contiguous shards of the genome with WIDE halos that are updated redundantly, refreshed once
per run_mcmc, and ONE all-gather of the per-branch J/D totals (+ accept count) per run_mcmc.

Why it is correct: one MH update of site i reads the paths of sites
i-2..i+2 and the cached triple log-likelihoods tri[i-1], tri[i+1]; it writes path i and
tri[i-1..i+1].  The RNG and the 3-colouring are keyed by the GLOBAL site index, so a
rank that holds copies of a neighbour's edge columns can update them itself and obtain
exactly what the owner computes.  Each colour phase, the two outermost still-valid halo
columns at every shard-internal edge lose a neighbour and go stale, so a halo of H
columns lasts H/2 phases = H/6 sweeps.  With H >= 6*(burn_in + batch) + 2 a whole
run_mcmc needs NO communication inside it: the halos are refreshed once before
reset(), and the statistics are combined once after it -- instead of 3 exchanges per
sweep.  The redundant work is 2H/n of a shard (0.1 % at n = 1e6, -L 10 -B 50).

Statistics.  J and D are exact 64-bit integers until the very end: J counts, every dwell time
of branch b is rint(dt * 2^k_b).  Every rank's run_mcmc returns the integer totals of its owned
sites per batch sweep; the ranks all-gather them in one fixed-size piece (with the accept count
in its tail), and every rank adds all pieces as integers and turns the sum into J, D once.
Integer sums do not depend on how they are grouped, so a sharded run reproduces the unsharded
one bit-for-bit on paths, states, J AND D, for any number of ranks and any cut points.

The reference has no parallelism at all (single-threaded); this
module is new capability, not a translation.
"""
import functools

import numpy as np

from . import host
from .host import FlatPaths
from .sampler import DeviceSampler, forward_to_dev
from .summaries import CHAIN, LIFECYCLE, NOUN, _per_sample, _window_range, summary_method

BLOCK = 256      # sites per block: halo widths and shard_cuts' cut points are whole blocks
TAIL = 1         # int64 words after a rank's counts in the all-gather: its accept count


def halo_width(sweeps_per_refresh):
    """halo columns that last `sweeps_per_refresh` sweeps, in whole 256-site blocks"""
    return max(BLOCK, -(-(6 * int(sweeps_per_refresh) + 2) // BLOCK) * BLOCK)


def shard_cuts(n_global, world, row_blocks=64):
    """cut points of `world` near-equal contiguous shards on multiples of 256 * row_blocks sites"""
    row = BLOCK * row_blocks
    cuts = [0] + [int(r * n_global / float(world) / row + 0.5) * row for r in range(1, world)] + [n_global]
    if any(b <= a for a, b in zip(cuts[:-1], cuts[1:])):
        raise ValueError("a genome of %d sites is too short for %d shards cut on %d sites" % (n_global, world, row))
    return cuts


def concat_sites(parts):
    """concatenate FlatPaths along the site axis"""
    B = parts[0].n_nodes - 1
    n = sum(p.n_sites for p in parts)
    init = np.concatenate([p.init.reshape(B, p.n_sites) for p in parts], axis=1)
    cnt = np.concatenate([p.counts().reshape(B, p.n_sites) for p in parts], axis=1)
    jumps = []
    for b in range(B):
        for p in parts:
            c = p.counts().reshape(B, p.n_sites)[b]
            o = p.offsets[:-1].reshape(B, p.n_sites)[b]
            jumps.append(p.jumps[int(o[0]):int(o[-1] + c[-1])])
    off = np.zeros(B * n + 1, np.uint64)
    off[1:] = np.cumsum(cnt.reshape(-1))
    return FlatPaths(n, parts[0].n_nodes, init.reshape(-1).copy(), off,
                     np.concatenate(jumps) if jumps else np.zeros(0))


class NullComm:
    """one rank: nothing to exchange, the gathered buffer IS the rank's piece"""
    rank, world = 0, 1

    def exchange(self, dev, send_left, recv_left, send_right, recv_right):
        pass

    def all_gather(self, dev, piece, gathered):
        assert gathered is piece


class TorchComm:
    """torch.distributed (backend "nccl" = RCCL over xGMI on the GPU box, "gloo" in the CPU
    tests).  The buffers are the device's own (DevBuf: device memory seen by torch through the
    CUDA array interface; the CPU double hands out numpy arrays), so nothing is staged: RCCL
    reads the packed columns where the kernels wrote them."""

    def __init__(self, dist, device=None):
        import torch
        self.dist, self.torch = dist, torch
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.device = device if device is not None else torch.device("cpu")
        # gloo cannot move GPU tensors: when several ranks SHARE one GPU to rehearse the N > 1
        # path on a 1-GPU box, device buffers are bounced through the host here (rehearsal only;
        # with the nccl backend RCCL reads and writes the device buffers directly)
        self.staged = self.device.type == "cuda" and dist.get_backend() == "gloo"

    def _t(self, buf):
        if hasattr(buf, "np"):                       # host buffer of the CPU device double
            return self.torch.from_numpy(buf.np)
        return self.torch.as_tensor(buf, device=self.device)   # zero-copy view of device memory

    def _sync(self):
        if self.device.type == "cuda":
            self.torch.cuda.synchronize(self.device)

    def exchange(self, dev, send_left, recv_left, send_right, recv_right):
        """swap halo buffers with the left/right neighbour (None = no neighbour on that side)"""
        dist = self.dist
        ops, back = [], []

        def add(send, recv, peer):
            ts, tr = self._t(send), self._t(recv)
            if self.staged:
                ts, dst = ts.cpu(), tr
                tr = self.torch.empty(tr.shape, dtype=tr.dtype)
                back.append((dst, tr))
            ops.append(dist.P2POp(dist.isend, ts, peer))
            ops.append(dist.P2POp(dist.irecv, tr, peer))

        if send_left is not None:
            add(send_left, recv_left, self.rank - 1)
        if send_right is not None:
            add(send_right, recv_right, self.rank + 1)
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        for dst, tmp in back:
            dst.copy_(tmp)
        self._sync()

    def all_gather(self, dev, piece, gathered):
        g, p = self._t(gathered), self._t(piece)
        if self.staged:
            outs = [self.torch.empty(p.shape, dtype=p.dtype) for _ in range(self.world)]
            self.dist.all_gather(outs, p.cpu())
            g.copy_(self.torch.cat(outs))
        elif self.device.type == "cuda":
            self.dist.all_gather_into_tensor(g, p)         # one RCCL all-gather, in place
        else:
            self.dist.all_gather(list(g.chunk(self.world)), p)
        self._sync()


def add_uint64(parts):
    """the sum of uint64 arrays of one shape; a sum that passes 64 bits is refused, not wrapped (the age sums of
    the lineage origin maps over wide windows near the sample cap)"""
    total = np.array(parts[0], np.uint64)
    for p in parts[1:]:
        t = total + np.asarray(p, np.uint64)
        if (t < total).any():
            raise OverflowError("a sum over contexts passes 64 bits: use narrower windows")
        total = t
    return total


class ShardedSampler:
    """SingleSiteSampler over a site-sharded genome.  `device_factory(device)` builds the
    per-rank engine (the HIP DeviceSampler / LocalGroup in the product; the tests inject an
    oracle-backed double to check the sharding logic on CPU with gloo)."""

    def __init__(self, comm, device=0, device_factory=None, direct_sampler=False, direct_fused=False):
        self.comm = comm
        if device_factory is None:
            device_factory = DeviceSampler
        self.dev = device_factory(device)
        # EPV_OPT_DIRECT_SAMPLER on this rank's engine (every context of a LocalGroup), set with the paths in setup()
        self.direct_sampler = bool(direct_sampler)
        # with direct_sampler: EPV_OPT_DIRECT_FUSED as well (the fused phase's direct bodies where it is eligible)
        self.direct_fused = bool(direct_fused)
        # a capacity overflow widens this shard's jump slots and the run carries on (as the
        # reference's vectors would); refresh_halos() brings all shards to the same width
        # before columns travel
        if hasattr(self.dev, "auto_grow"):
            self.dev.auto_grow = True
        self.halo = 0
        self._halo_bufs, self._halo_bytes = None, 0
        self._piece = self._gathered = None
        self._piece_batch = 0
        self._regions, self._n_fixed = None, 0

    def set_regions(self, lengths):
        """genomic regions of the whole genome (SingleSiteSampler.set_regions), the same on every rank: this rank's
        engine gets the slice of the genome's mask of fixed sites for its local columns, halos included.  Kept and
        applied again by setup(); None clears.  run_mcmc's acceptance rate counts the sites that can be updated"""
        self._regions = None if lengths is None else [int(m) for m in lengths]
        if not getattr(self, "n_loc", 0):
            return
        if self._regions is None:
            self._n_fixed = 0
            return self.dev.set_fixed_sites(None)
        whole = host.region_fixed_mask(self.n_global, self._regions)
        self._n_fixed = int(whole[1:-1].sum())
        self.dev.set_fixed_sites(whole[self.g0:self.g0 + self.n_loc])

    def owned_sites(self):
        return self.n_own - (1 if self.comm.rank == 0 else 0) - \
            (1 if self.comm.rank == self.comm.world - 1 else 0)

    def setup(self, model, tree, fp_own, cuts, capacity=16, sweeps_per_refresh=60):
        """fp_own: this rank's owned columns, sites [cuts[rank], cuts[rank+1]) of the genome
        (cuts as shard_cuts makes them, or any others whose shards hold their halos).  The halo
        is sized for `sweeps_per_refresh` sweeps between refreshes."""
        c = self.comm
        cuts = [int(x) for x in cuts]
        if len(cuts) != c.world + 1 or cuts[0] != 0:
            raise ValueError("cuts must list world + 1 cut points starting at 0")
        n_own, n_global = cuts[c.rank + 1] - cuts[c.rank], cuts[-1]
        if fp_own.n_sites != n_own:
            raise ValueError("fp_own has %d sites, the cuts give this rank %d" % (fp_own.n_sites, n_own))
        self.cuts = cuts
        self.n_own, self.n_global, self.B = n_own, n_global, tree.n_nodes - 1
        H = halo_width(sweeps_per_refresh) if c.world > 1 else 0
        if H > min(b - a for a, b in zip(cuts[:-1], cuts[1:])):
            raise ValueError("a shard is smaller than the %d-column halo" % H)
        self.halo = H
        left = H if c.rank > 0 else 0
        right = H if c.rank < c.world - 1 else 0
        parts = []
        if left:
            parts.append(fp_own.slice_sites(0, H))               # placeholder, refreshed below
        parts.append(fp_own)
        if right:
            parts.append(fp_own.slice_sites(n_own - H, n_own))
        fp_loc = concat_sites(parts) if len(parts) > 1 else fp_own
        self.n_loc = fp_loc.n_sites
        self.left, self.right = left, right
        self.g0 = cuts[c.rank] - left
        self.dev.set_tree(tree)
        self.dev.set_model(model)
        self.dev.upload_paths(fp_loc, capacity, self.g0, n_global)
        if self.direct_sampler and self.direct_fused:
            self.dev.set_direct_sampler(True, fused=True)
        elif self.direct_sampler:
            self.dev.set_direct_sampler(True)
        self.dev.set_halo(left, right)
        if getattr(self, "_regions", None) is not None:
            self.set_regions(self._regions)
        self.refresh_halos()

    def _agree_on_capacity(self):
        """packed columns have capacity-dependent size: all ranks move to the widest"""
        if self.comm.world == 1 or not hasattr(self.dev, "capacity"):
            return
        piece, gathered = self.dev.alloc(8), self.dev.alloc(8 * self.comm.world)
        self.dev.write(piece, 0, np.array([float(self.dev.capacity())]))
        self.comm.all_gather(self.dev, piece, gathered)
        cap = int(self.dev.read(gathered, 0, self.comm.world).max())
        piece.free()
        gathered.free()
        if cap != self.dev.capacity():
            self.dev.set_capacity(cap)

    def refresh_halos(self):
        """ship my H outermost owned columns to each neighbour; take theirs as my halos"""
        if self.comm.world == 1:
            return
        self._agree_on_capacity()
        H = self.halo
        nbytes = H * self.dev.column_bytes()
        if self._halo_bufs is None or self._halo_bytes != nbytes:
            for b in self._halo_bufs or []:
                b.free()
            self._halo_bufs, self._halo_bytes = [self.dev.alloc(nbytes) for _ in range(4)], nbytes
        sl, rl, sr, rr = self._halo_bufs
        if self.left:
            self.dev.pack_columns(self.left, H, sl)
        if self.right:
            self.dev.pack_columns(self.n_loc - self.right - H, H, sr)
        self.comm.exchange(self.dev, sl if self.left else None, rl if self.left else None,
                           sr if self.right else None, rr if self.right else None)
        if self.left:
            self.dev.unpack_columns(0, H, rl)
        if self.right:
            self.dev.unpack_columns(self.n_loc - H, H, rr)
        self.dev.set_halo(self.left, self.right)     # marks the halos fresh

    # ---- SingleSiteSampler interface
    def reset(self):
        """refresh the halos (they are stale after the previous run_mcmc), then cache the
        triple log-likelihoods as SingleSiteSampler::reset does"""
        self.refresh_halos()
        self.dev.reset()

    def sweeps(self, n_sweeps, seed, sweep_base=0):
        """n plain sweeps (the epievo_sim_pairwise loop), refreshing halos as needed"""
        nacc, done = 0, 0
        while done < n_sweeps:
            k = min(n_sweeps - done, self.dev.halo_phases_left() // 3) if self.comm.world > 1 \
                else n_sweeps - done
            if k == 0:
                self.refresh_halos()
                self.dev.reset()
                continue
            nacc += self.dev.sweep(k, seed, sweep_base + done)
            done += k
        return nacc

    def run_mcmc(self, burn_in, batch, seed, sweep_base=0):
        """-> (J, D, acc_rate): batch averages over the WHOLE genome, identical on every rank
        and bit-identical to the unsharded run"""
        if self.comm.world > 1 and self.dev.halo_phases_left() < 3 * (burn_in + batch):
            raise RuntimeError("halo too narrow for %d sweeps: call reset() first or set up with "
                               "a larger sweeps_per_refresh" % (burn_in + batch))
        words = batch * self.B * 16 + TAIL
        if self._piece is None or self._piece_batch != batch:
            for b in {id(x): x for x in (self._piece, self._gathered) if x is not None}.values():
                b.free()
            self._piece = self.dev.alloc(words * 8)
            self._gathered = self.dev.alloc(words * 8 * self.comm.world) if self.comm.world > 1 \
                else self._piece
            self._piece_batch = batch
        # this rank's integer totals with its accept count in the tail of the same piece, so ONE
        # collective per EM iteration carries everything
        counts, nacc = self.dev.run_mcmc_counts(burn_in, batch, seed, sweep_base)
        self.dev.write(self._piece, 0, np.append(counts.reshape(-1), np.int64(nacc)))
        self.comm.all_gather(self.dev, self._piece, self._gathered)
        pieces = self.dev.read(self._gathered, 0, words * self.comm.world, np.int64).reshape(self.comm.world, words)
        total = pieces.sum(axis=0, dtype=np.int64)
        J, D = self.dev.counts_to_stats(total[:-TAIL].reshape(batch, -1), batch, True)
        return J, D, float(total[-TAIL]) / float(batch * (self.n_global - 2 - getattr(self, "_n_fixed", 0)))

    # ---- the posterior summaries: every rank counts its owned columns, and a read-out of
    # the whole genome, identical on every rank, has one of three shapes across ranks: _gather_sites, _gather_sums,
    # _gather_parts.  At one rank none of them makes a collective
    def _gather_words(self, mine):
        """all-gather equal-sized uint32 pieces -> [world, words]"""
        words = len(mine)
        piece, gathered = self.dev.alloc(4 * words), self.dev.alloc(4 * words * self.comm.world)
        try:
            self.dev.write(piece, 0, mine)
            self.comm.all_gather(self.dev, piece, gathered)
            return self.dev.read(gathered, 0, words * self.comm.world, np.uint32).reshape(self.comm.world, words)
        finally:
            piece.free()
            gathered.free()

    def _gather_sites(self, ns, blocks, noun, extra=()):
        """rows concatenated by site in genome order, ONE collective.  blocks: this rank's uint32 arrays [rows, its
        sites, words per cell] -> (the same over the whole genome, the ranks' `extra` words [world, len(extra)]).  A
        rank's piece: its blocks, each padded to the sites of the widest rank, then the sample count (two words),
        then `extra`"""
        world = self.comm.world
        if world == 1:
            return blocks, np.array([extra], np.uint32)
        sizes = [b - a for a, b in zip(self.cuts[:-1], self.cuts[1:])]
        m, cnt = max(sizes), blocks[0].shape[1]
        if cnt != sizes[self.comm.rank]:
            raise RuntimeError("this rank counts %d sites, it owns %d" % (cnt, sizes[self.comm.rank]))
        tail = np.array([ns & 0xffffffff, ns >> 32] + list(extra), np.uint32)
        mine = []
        for b in blocks:
            padded = np.zeros((b.shape[0], m, b.shape[2]), np.uint32)
            padded[:, :cnt] = b
            mine.append(padded.reshape(-1))
        allw = self._gather_words(np.concatenate(mine + [tail]))
        at = allw.shape[1] - len(tail)
        if any(int(w[at]) | (int(w[at + 1]) << 32) != ns for w in allw):
            raise RuntimeError("the ranks hold different numbers of %s samples" % noun)
        out, lo = [], 0
        for b in blocks:
            hi = lo + b.shape[0] * m * b.shape[2]
            out.append(np.concatenate([allw[r, lo:hi].reshape(b.shape[0], m, b.shape[2])[:, :sizes[r]]
                                       for r in range(world)], axis=1))
            lo = hi
        return out, allw[:, at + 2:]

    def _gather_sums(self, ns, arrays, noun, add=None):
        """integer totals added, ONE collective.  arrays: this rank's contributions, 64-bit integers of one dtype and
        of the same shapes on every rank -> their sums over the ranks (`add` of the ranks' arrays, in rank order; plain
        wrapping addition unless given).  A rank's piece: the arrays, then the sample count"""
        if self.comm.world == 1:
            return arrays
        dt = arrays[0].dtype
        mine = np.concatenate([np.asarray(a, dt).reshape(-1) for a in arrays] + [np.array([ns], dt)])
        allw = np.ascontiguousarray(self._gather_words(mine.view(np.uint32))).view(dt)
        if any(int(w[-1]) != ns for w in allw):
            raise RuntimeError("the ranks hold different numbers of %s samples" % noun)
        out, lo = [], 0
        for a in arrays:
            parts = [w[lo:lo + a.size].reshape(a.shape) for w in allw]
            out.append(add(parts) if add else np.sum(parts, axis=0, dtype=dt))
            lo += a.size
        return out

    def _gather_parts(self, ns, arrays, noun, merge):
        """parts merged in genome order, TWO collectives: the sample counts are compared first (a part's size depends
        on them), then the ranks' parts, uint64 arrays of the same shapes on every rank, are all-gathered and
        merge([(arrays of rank 0), (arrays of rank 1), ...]) is the part of the whole genome"""
        if self.comm.world == 1:
            return tuple(arrays)
        counts = self._gather_words(np.array([ns & 0xffffffff, ns >> 32], np.uint32))
        if any(int(w[0]) | (int(w[1]) << 32) != ns for w in counts):
            raise RuntimeError("the ranks hold different numbers of %s samples" % noun)
        mine = np.concatenate([a.reshape(-1) for a in arrays]).astype(np.uint64)
        allw = np.ascontiguousarray(self._gather_words(mine.view(np.uint32))).view(np.uint64)
        ends = np.cumsum([a.size for a in arrays])
        return merge([tuple(w[e - a.size:e].reshape(a.shape) for a, e in zip(arrays, ends)) for w in allw])

    def path_average(self, counts=False):
        """-> (samples, [N-1, n_global, P]) of the whole genome, identical on every rank: the ranks'
        counts are all-gathered (one collective) and concatenated in genome order"""
        ns, own = self.dev.path_average(counts=True)
        (own,), _ = self._gather_sites(ns, [own], NOUN["path_average"])
        return ns, _per_sample(own, ns, counts)

    def branch_events(self, counts=False):
        """-> (samples, [6, N-1, n_global]) of the whole genome, identical on every rank: the ranks'
        planes are all-gathered (one collective) and concatenated in genome order"""
        ns, own = self.dev.branch_events(counts=True)
        (rows,), _ = self._gather_sites(ns, [own.reshape(-1, own.shape[2], 1)], NOUN["branch_events"])
        return ns, _per_sample(rows.reshape(own.shape[0], own.shape[1], -1), ns, counts)

    def branch_event_windows(self, W):
        """-> (samples, uint64 [6, N-1, windows]) of the whole genome, identical on every rank: the ranks'
        contributions (windows of global sites) are all-gathered and summed"""
        ns, own = self.dev.branch_event_windows(W)
        return ns, self._gather_sums(ns, [own], NOUN["branch_events"])[0]

    def change_patterns(self, counts=False):
        """-> (samples, [R, n_global]) of the whole genome, identical on every rank: the ranks' rows are
        all-gathered (one collective) and concatenated in genome order"""
        ns, own = self.dev.change_patterns(counts=True)
        (rows,), _ = self._gather_sites(ns, [own[:, :, None]], NOUN["change_patterns"])
        return ns, _per_sample(rows[:, :, 0], ns, counts)

    def change_pattern_windows(self, W):
        """-> (samples, uint64 [R, windows]) of the whole genome, identical on every rank: the ranks'
        contributions (windows of global sites) are all-gathered and summed"""
        ns, own = self.dev.change_pattern_windows(W)
        return ns, self._gather_sums(ns, [own], NOUN["change_patterns"])[0]

    def window_stats(self, counts=False):
        """-> (samples, J, D [nw, N-1, 8]) of the whole genome (or the int64 [nw, N-1, 16]), identical on
        every rank: the ranks' integer contributions are all-gathered and added, then converted once"""
        ns, own = self.dev.window_counts()
        own, = self._gather_sums(ns, [own], NOUN["window_stats"])
        if counts:
            return ns, own
        if not ns:
            raise RuntimeError("window statistics hold no sample")
        return (ns,) + self.dev.window_counts_to_stats(own, ns)

    def epoch_stats(self, counts=False):
        """-> (samples, J, D [N-1, P, 8]) of the whole genome (or the closed integers), identical on every
        rank: the ranks' raw parts are all-gathered and added as integers, then closed once"""
        ns, own = self.dev.epoch_raw()
        own, = self._gather_sums(ns, [own], NOUN["epoch_stats"], host.epoch_raw_add)
        _, k, fixT = self.dev.epoch_stats_layout()
        return host.epoch_finish(own, fixT, k, ns, counts)

    def lineage_origins(self, counts=False):
        """-> (samples, rows [R, 2], origin [R, n_global], age [L, n_global]) of the whole genome, identical on
        every rank: the ranks' cells are all-gathered (one collective) and concatenated in genome order; an age cell
        travels as two words, and the scale exponent after the sample count"""
        ns, rows, origin, age = self.dev.lineage_origins(counts=True)
        k = self.dev.lineage_origins_scale_exp()
        age_words = np.ascontiguousarray(age, np.uint64).view(np.uint32).reshape(age.shape[0], -1, 2)
        (origin, age_words), ks = self._gather_sites(ns, [origin[:, :, None], age_words], NOUN["lineage_origins"],
                                                     extra=[k & 0xffffffff])
        if any(int(w[0]) != k & 0xffffffff for w in ks):
            raise RuntimeError("the ranks hold lineage-origin ages of different scales")
        origin, age = origin[:, :, 0], np.ascontiguousarray(age_words).view(np.uint64)[:, :, 0]
        if counts:
            return ns, rows, origin, age
        d = float(ns) if ns else 1.0
        return ns, rows, origin / d, np.ldexp(age.astype(np.float64), -k) / d

    def lineage_origin_windows(self, W):
        """-> (samples, uint64 [R, windows], uint64 [L, windows]) of the whole genome, identical on every rank:
        the ranks' contributions (windows of global sites) are all-gathered and added as integers"""
        ns, ow, aw = self.dev.lineage_origin_windows(W)
        ow, aw = self._gather_sums(ns, [ow, aw], NOUN["lineage_origins"], add_uint64)
        return ns, ow, aw

    def domain_stats_part(self):
        """-> (samples, hist, len_sum, edges): the part of the whole genome, identical on every rank: the sample
        counts are compared first (a part's size depends on them), then the ranks' parts are all-gathered and
        merged in genome order"""
        ns, *part = self.dev.domain_stats_part()
        return (ns,) + self._gather_parts(ns, part, NOUN["domain_stats"], host.domain_parts_merge)

    def domain_stats(self):
        """-> (samples, hist [N, 2, 128], len_sum [N, 2]) of the whole genome, closed; every rank merges and closes"""
        ns, hist, len_sum, edges = self.domain_stats_part()
        return (ns,) + host.domain_part_close(hist, len_sum, edges)

    def domain_turnover_part(self):
        """-> (samples, hist, len_sum, edges): the part of the whole genome, identical on every rank: the sample
        counts are compared first (a part's size depends on them), then the ranks' parts are all-gathered and
        merged in genome order"""
        ns, *part = self.dev.domain_turnover_part()
        return (ns,) + self._gather_parts(ns, part, NOUN["domain_turnover"], host.turnover_parts_merge)

    def domain_turnover(self):
        """-> (samples, hist [R, 2, 2, 128], len_sum [R, 2, 2]) of the whole genome, closed; every rank merges and
        closes"""
        ns, hist, len_sum, edges = self.domain_turnover_part()
        return (ns,) + host.turnover_part_close(hist, len_sum, edges)

    def spatial_correlation_part(self):
        """-> (samples, sites, n11, edges): the part of the whole genome, identical on every rank: the sample counts
        are compared first (a part's size depends on them), then the ranks' parts, each behind its number of sites,
        are all-gathered and merged in genome order"""
        ns, cnt, n11, edges = self.dev.spatial_correlation_part()
        if self.comm.world == 1:
            return ns, cnt, n11, edges
        return (ns,) + self._gather_parts(
            ns, [np.array([cnt], np.uint64), n11, edges], NOUN["spatial_correlation"],
            lambda parts: host.corr_parts_merge([(int(c[0]), a, e) for c, a, e in parts]))

    def spatial_correlation(self):
        """-> (samples, n11, left1, right1), each [R, L + 1], of the whole genome, closed; every rank merges and
        closes"""
        ns, cnt, n11, edges = self.spatial_correlation_part()
        return (ns,) + host.corr_part_close(cnt, n11, edges)

    def domain_maps_part(self):
        """-> (samples, sites, counts, edges): the part of the whole genome, identical on every rank: the sample counts
        are compared first (a part's size depends on them), then the ranks' parts, each behind its number of sites
        and with its counts padded to the sites of the widest rank, are all-gathered and merged in genome order"""
        ns, cnt, counts, edges = self.dev.domain_maps_part()
        if self.comm.world == 1:
            return ns, cnt, counts, edges
        sizes = self.dev.domain_maps_layout()[1]
        widest = max(b - a for a, b in zip(self.cuts[:-1], self.cuts[1:]))
        padded = np.zeros(counts.shape[:2] + (widest,), np.uint64)
        padded[:, :, :cnt] = counts
        return (ns,) + self._gather_parts(
            ns, [np.array([cnt], np.uint64), padded, edges], NOUN["domain_maps"],
            lambda parts: host.domain_maps_merge(
                sizes, [(int(c[0]), a[:, :, :int(c[0])].astype(np.uint32), e) for c, a, e in parts]))

    def domain_maps(self, counts=False):
        """-> (samples, maps [N, K, n_global]) of the whole genome; every rank merges"""
        ns, _, c, _ = self.domain_maps_part()
        return ns, _per_sample(c, ns, counts)

    def change_tracts_part(self):
        """-> (samples, hist, len_sum, edges): the part of the whole genome, identical on every rank: the sample
        counts are compared first (a part's size depends on them), then the ranks' parts are all-gathered and
        merged in genome order"""
        ns, *part = self.dev.change_tracts_part()
        return (ns,) + self._gather_parts(ns, part, NOUN["change_tracts"], host.tract_parts_merge)

    def change_tracts(self):
        """-> (samples, hist [B, 27, 128], len_sum [B, 27]) of the whole genome, closed; every rank merges and closes"""
        ns, hist, len_sum, edges = self.change_tracts_part()
        return (ns,) + host.tract_part_close(hist, len_sum, edges)

    def mixing(self, counts=False):
        """-> DeviceSampler.mixing of the whole genome, identical on every rank: the ranks' rows are all-gathered
        (one collective) and concatenated in genome order (a 64-bit cell travels as two words); the ranks' pair
        counts travel behind the sample count and must agree"""
        ns, mp, pairs, moved, S1, S2, Ck = self.dev.mixing(counts=True)
        wide = np.ascontiguousarray(np.concatenate([S1[None], S2[None], Ck]), np.uint64)
        tail = np.concatenate([[mp], pairs]).astype(np.uint64).view(np.uint32)
        (moved, wide), tails = self._gather_sites(
            ns, [moved[None, :, None], wide.view(np.uint32).reshape(wide.shape[0], -1, 2)], NOUN["mixing"], extra=list(tail))
        if any(not np.array_equal(w, tail) for w in tails):
            raise RuntimeError("the ranks hold mixing samples of different runs (their pair counts differ)")
        wide = np.ascontiguousarray(wide).view(np.uint64)[:, :, 0]
        out = (ns, mp, pairs, np.ascontiguousarray(moved[0, :, 0]), wide[0], wide[1], wide[2:])
        return out if counts else host.mixing_summary(*out)

    def mixing_windows(self, W):
        """-> (samples, moved_pairs, uint64 [windows]) of the whole genome, identical on every rank: the ranks'
        contributions (windows of global sites) are all-gathered and summed"""
        ns, mp, own = self.dev.mixing_windows(W)
        return ns, mp, self._gather_sums(ns, [own], NOUN["mixing"])[0]

    def owned_paths(self):
        return self.dev.paths().slice_sites(self.left, self.n_loc - self.right)


# what needs nothing from the other ranks is the engine's own
forward_to_dev(ShardedSampler, LIFECYCLE + [
    "set_model", "scale_jump_times", "window_stats_scale_exps", "lineage_origins_layout", "lineage_origin_rows",
    "lineage_origins_scale_exp", "domain_stats_layout", "domain_turnover_layout", "spatial_correlation_layout",
    "mixing_layout", "domain_maps_layout", "change_tracts_layout"])


class LocalGroup:
    """Two or three shards on ONE GPU behind the DeviceSampler interface.

    The three kernels of a colour phase depend on each other, so on one stream every launch
    pays its own ramp and tail.  Two contexts on the same device, each owning half of the
    (local) genome plus redundant halos exactly like shards on different GPUs, run on their own
    streams from their own host threads and fill each other's gaps: +17 % on one MI355X
    (tools/probe_streams.py).  The group reproduces the single-context run bit-for-bit
    INCLUDING D: every shard returns the integer totals of its owned sites and the group adds
    them (epv_run_mcmc_counts / epv_counts_to_stats).  Drop-in for DeviceSampler inside
    ShardedSampler, so it composes with the multi-GPU sharding."""

    BLOCK = 256

    def __init__(self, device=0, shards=2, sweeps_per_refresh=60):
        from concurrent.futures import ThreadPoolExecutor
        self.device, self.k_req = device, max(1, int(shards))
        self.H_INT = halo_width(sweeps_per_refresh)   # internal halo columns (whole blocks)
        self.subs = [DeviceSampler(device) for _ in range(self.k_req)]
        self.pool = ThreadPoolExecutor(max_workers=self.k_req)
        self.n_sites = self.n_nodes = self.B = 0
        self.capacity_events = []
        self._auto_grow = False
        self.outer = (0, 0)
        self.halo_mode = False

    # ---- plumbing
    @property
    def auto_grow(self):
        return self._auto_grow

    @auto_grow.setter
    def auto_grow(self, v):
        self._auto_grow = bool(v)
        for s in self.subs:
            s.auto_grow = bool(v)

    def close(self):
        if getattr(self, "_closed", False):
            return
        self._closed = True
        for s in self.subs:
            s.close()
        self.pool.shutdown(wait=True)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _each(self, fn):
        """run fn(j, sub) for every shard from its own host thread; results in shard order"""
        if len(self.subs) == 1:
            return [fn(0, self.subs[0])]
        return [f.result() for f in [self.pool.submit(fn, j, s) for j, s in enumerate(self.subs)]]

    def set_tree(self, tree):
        self.n_nodes, self.B = tree.n_nodes, tree.n_nodes - 1
        for s in self.subs:
            s.set_tree(tree)

    def set_model(self, model):
        for s in self.subs:
            s.set_model(model)

    def upload_paths(self, fp, capacity=0, global_site_offset=0, n_global=None):
        n, H, Q = fp.n_sites, self.H_INT, self.BLOCK
        k = self.k_req
        while k > 1 and n < k * (2 * H + 2 * Q):      # every shard must own more than its halos
            k -= 1
        for s in self.subs[k:]:
            s.close()
        self.subs = self.subs[:k]
        cuts = [0] + [int(round(j * n / float(k) / Q)) * Q for j in range(1, k)] + [n]
        self.a, self.b = cuts[:-1], cuts[1:]                       # pieces of [0, n)
        self.lo = [a - (H if j > 0 else 0) for j, a in enumerate(self.a)]
        self.hi = [b + (H if j < k - 1 else 0) for j, b in enumerate(self.b)]
        if capacity == 0:
            capacity = int(max(16, 2 * (fp.counts().max() if n else 0) + 8))
        n_global = global_site_offset + n if n_global is None else n_global
        for j, s in enumerate(self.subs):
            s.upload_paths(fp.slice_sites(self.lo[j], self.hi[j]) if k > 1 else fp, capacity,
                           global_site_offset + self.lo[j], n_global)
        self.n_sites = n
        self.halo_mode = False
        self.outer = (0, 0)     # the halos are set by set_halo() (ShardedSampler) or by reset()
        self._g0, self._n_global = int(global_site_offset), int(n_global)
        if getattr(self, "_regions", None) is not None:     # (new paths cleared the shards' masks)
            self.set_regions(self._regions)

    # ---- fixed sites and regions: every shard gets the slice of the mask for its local columns, halos included,
    # so a halo column that its owner holds fixed is held fixed in the copy too
    def set_fixed_sites(self, mask):
        """as DeviceSampler.set_fixed_sites over the group's columns; None clears"""
        if mask is None:
            for s in self.subs:
                s.set_fixed_sites(None)
            return
        m = (np.ascontiguousarray(mask).reshape(-1) != 0).astype(np.uint8)
        if m.size != self.n_sites:
            raise ValueError("mask of fixed sites: %d entries for %d sites" % (m.size, self.n_sites))
        for j, s in enumerate(self.subs):
            s.set_fixed_sites(m if len(self.subs) == 1 else m[self.lo[j]:self.hi[j]])

    def fixed_sites(self):
        """the fixed sites among those whose acceptances are counted: the shards' numbers added"""
        return sum(s.fixed_sites() for s in self.subs)

    def set_regions(self, lengths):
        """genomic regions of the whole genome (SingleSiteSampler.set_regions): their end sites are held fixed.  Kept
        and re-applied to new paths; None clears"""
        self._regions = None if lengths is None else [int(m) for m in lengths]
        if not self.n_sites:
            return
        if self._regions is None:
            return self.set_fixed_sites(None)
        whole = host.region_fixed_mask(self._n_global, self._regions)
        self.set_fixed_sites(whole[self._g0:self._g0 + self.n_sites])

    # ---- halos
    def set_halo(self, left, right):
        """outer halo blocks of the whole group (multi-GPU); the internal ones are managed here"""
        self.outer, self.halo_mode = (left, right), True
        k, H = len(self.subs), self.H_INT
        for j, s in enumerate(self.subs):
            s.set_halo(left if j == 0 else H, right if j == k - 1 else H)

    def halo_phases_left(self):
        return min(s.halo_phases_left() for s in self.subs)

    def _locate(self, first, count):
        for j in range(len(self.subs)):
            if self.a[j] <= first < self.b[j]:
                if first + count > self.hi[j]:
                    raise ValueError("column range straddles two shards of the group")
                return j, first - self.lo[j]
        raise ValueError("bad column range")

    def column_bytes(self):
        return self.subs[0].column_bytes()

    # buffers live on the group's GPU; any context can allocate and fill them
    def alloc(self, nbytes):
        return self.subs[0].alloc(nbytes)

    def write(self, buf, offset, arr):
        self.subs[0].write(buf, offset, arr)

    def read(self, buf, offset, count, dtype=np.float64):
        return self.subs[0].read(buf, offset, count, dtype)

    def pack_columns(self, first, count, buf):
        j, f = self._locate(first, count)
        self.subs[j].pack_columns(f, count, buf)

    def unpack_columns(self, first, count, buf):
        j, f = self._locate(first, count)
        self.subs[j].unpack_columns(f, count, buf)

    def get_columns(self, first, count):
        j, f = self._locate(first, count)
        return self.subs[j].get_columns(f, count)

    def put_columns(self, first, count, buf):
        j, f = self._locate(first, count)
        self.subs[j].put_columns(f, count, buf)

    def _refresh_internal(self):
        k, H = len(self.subs), self.H_INT
        cap = max(s.capacity() for s in self.subs)
        for s in self.subs:
            if s.capacity() != cap:
                s.set_capacity(cap)
        for j in range(k - 1):
            L, R = self.subs[j], self.subs[j + 1]
            L.copy_columns_to(self.b[j] - H - self.lo[j], H, R, 0)          # L's edge -> R's left halo
            R.copy_columns_to(H, H, L, self.b[j] - self.lo[j])              # R's edge -> L's right halo
        if k > 1:
            self.set_halo(*self.outer)                                      # marks them fresh

    # ---- the SingleSiteSampler surface
    def reset(self):
        self._refresh_internal()
        self._each(lambda j, s: s.reset())

    def _sweep_all(self, k, seed, sweep_base):
        nacc = sum(self._each(lambda j, s: s.sweep(k, seed, sweep_base)))
        # the shards update their shared halo columns redundantly: after an absorbed overflow
        # they must go on proposing under ONE capacity, or one accepts what the other rejects
        if len(self.subs) > 1 and len({s.capacity() for s in self.subs}) > 1:
            self.set_capacity(max(s.capacity() for s in self.subs))
        for s in self.subs:
            self.capacity_events += s.capacity_events
            s.capacity_events = []
        return nacc

    def sweep(self, n_sweeps, seed, sweep_base=0):
        if len(self.subs) > 1 and self.halo_phases_left() < 3 * n_sweeps:
            done = 0
            nacc = 0
            while done < n_sweeps:
                kk = min(n_sweeps - done, self.halo_phases_left() // 3)
                if kk == 0:
                    self.reset()
                    continue
                nacc += self._sweep_all(kk, seed, sweep_base + done)
                done += kk
            return nacc
        return self._sweep_all(n_sweeps, seed, sweep_base)

    def run_mcmc_counts(self, burn_in, batch, seed, sweep_base=0):
        """as DeviceSampler.run_mcmc_counts over the group's owned sites: the shards' totals added"""
        if self.halo_phases_left() < 3 * (burn_in + batch) and len(self.subs) > 1:
            raise RuntimeError("internal halo of %d columns is too narrow for %d sweeps without a "
                               "reset()" % (self.H_INT, burn_in + batch))
        if getattr(self, "_corr_lag", 0):
            # a shard that owns fewer than max_lag sites refuses here, before any shard's first sweep
            self._each(lambda j, s: s.spatial_correlation_layout())
        if getattr(self, "_dmaps_on", False):
            # likewise a shard that owns fewer sites than an edge record of the domain maps holds
            self._each(lambda j, s: s.domain_maps_layout())
        res = self._each(lambda j, s: s.run_mcmc_counts(burn_in, batch, seed, sweep_base))
        for s in self.subs:
            self.capacity_events += s.capacity_events
            s.capacity_events = []
        return sum(c for c, _ in res), sum(n for _, n in res)

    def counts_to_stats(self, counts, batch, average=True):
        return self.subs[0].counts_to_stats(counts, batch, average)

    def run_mcmc(self, burn_in, batch, seed, sweep_base=0, average=True):
        if len(self.subs) == 1 and not self.halo_mode:
            return self.subs[0].run_mcmc(burn_in, batch, seed, sweep_base, average)
        counts, nacc = self.run_mcmc_counts(burn_in, batch, seed, sweep_base)
        J, D = self.counts_to_stats(counts, batch, average)
        return J, D, nacc

    def scale_jump_times(self, new_branches):
        for s in self.subs:
            s.scale_jump_times(new_branches)

    def _owned_slices(self):
        k = len(self.subs)
        return [(0 if j == 0 else self.a[j] - self.lo[j], self.b[j] - self.lo[j]) for j in range(k)]

    def paths(self):
        if len(self.subs) == 1:
            return self.subs[0].paths()
        ps = self._each(lambda j, s: s.paths())
        return concat_sites([p.slice_sites(lo, hi) for p, (lo, hi) in zip(ps, self._owned_slices())])

    def tri_llh(self):
        ts = [s.tri_llh() for s in self.subs]
        return np.concatenate([t[lo:hi] for t, (lo, hi) in zip(ts, self._owned_slices())])

    def capacity(self):
        return max(s.capacity() for s in self.subs)

    def set_capacity(self, capacity):
        for s in self.subs:
            s.set_capacity(capacity)

    # ---- the posterior summaries: every shard counts the sites it owns.  enable_<stem>,
    # reset_<stem>, accumulate_<stem> and <stem>_samples of every row of SUMMARIES and DIAGNOSTICS are made below the class of the
    # three helpers here (enable_spatial_correlation is written out: it keeps the lag).  A read-out takes every
    # shard's, wants the same number of samples of all, and concatenates along sites, adds integers or merges parts
    def _each_call(self, name, *args, **kwargs):
        """every shard's method `name`, from the shard's own host thread; results in shard (= genome) order"""
        return self._each(lambda j, s: getattr(s, name)(*args, **kwargs))

    def _reset_summary(self, s):
        self._each_call("reset_" + s.stem)

    def _accumulate_summary(self, s):
        if len(self.subs) > 1 and not self.halo_mode:
            # before the first reset() the shards' ranges overlap (their halos are not marked yet)
            raise RuntimeError("reset() the group before taking %s %s sample" % (s.article, s.noun))
        self._each_call("accumulate_" + s.stem)

    def _summary_samples(self, s):
        return getattr(self.subs[0], s.stem + "_samples")()

    def _same_samples(self, parts, noun):
        ns = parts[0][0]
        if any(p[0] != ns for p in parts):
            raise RuntimeError("the shards of the group hold different numbers of %s samples" % noun)
        return ns

    def _parts(self, stem, name, *args, **kwargs):
        """-> (the number of samples all shards agree on, every shard's read-out `name` of the summary `stem`)"""
        parts = self._each_call(name, *args, **kwargs)
        return self._same_samples(parts, NOUN[stem]), parts

    @staticmethod
    def _along_sites(parts, field, axis=1):
        return np.concatenate([p[field] for p in parts], axis=axis)

    @staticmethod
    def _added(parts, field, add=sum):
        return add([p[field] for p in parts])

    @staticmethod
    def _merged(parts, merge):
        return merge([p[1:] for p in parts])

    def _layout_over_shards(self, name):
        """a layout (.., .., first local site, sites, ..): of the first shard, with the sites of all shards"""
        lay = self._each_call(name)
        return lay[0][:3] + (sum(v[3] for v in lay),) + lay[0][4:]

    def _windows(self, W, first_window, n_windows):
        return _window_range(W, self.subs[0].n_global, first_window, n_windows)

    # average history of the sampled paths
    def path_average(self, counts=False):
        """-> (samples, [N-1, sites, P]) over the group's owned sites, shards in genome order"""
        ns, parts = self._parts("path_average", "path_average", counts=True)
        return ns, _per_sample(self._along_sites(parts, 1), ns, counts)

    # posterior branch-event maps
    def branch_events(self, counts=False):
        """-> (samples, [6, N-1, sites]) over the group's owned sites, shards in genome order"""
        ns, parts = self._parts("branch_events", "branch_events", counts=True)
        return ns, _per_sample(self._along_sites(parts, 1, axis=2), ns, counts)

    def branch_event_windows(self, W, first_window=0, n_windows=None):
        """-> (samples, uint64 [6, N-1, windows]): the shards' contributions to the windows of W global
        sites, added"""
        W, n_windows = self._windows(W, first_window, n_windows)
        ns, parts = self._parts("branch_events", "branch_event_windows", W, first_window, n_windows)
        return ns, self._added(parts, 1)

    # change patterns
    def change_patterns(self, counts=False):
        """-> (samples, [R, sites]) over the group's owned sites, shards in genome order"""
        ns, parts = self._parts("change_patterns", "change_patterns", counts=True)
        return ns, _per_sample(self._along_sites(parts, 1), ns, counts)

    def change_pattern_windows(self, W, first_window=0, n_windows=None):
        """-> (samples, uint64 [R, windows]): the shards' contributions to the windows of W global sites,
        added"""
        W, n_windows = self._windows(W, first_window, n_windows)
        ns, parts = self._parts("change_patterns", "change_pattern_windows", W, first_window, n_windows)
        return ns, self._added(parts, 1)

    # regional sufficient statistics: every shard adds the windows its owned sites meet
    def window_counts(self, first_window=0, n_windows=None):
        """-> (samples, int64 [windows, N-1, 16]): the shards' contributions, added as integers"""
        ns, parts = self._parts("window_stats", "window_counts", first_window, n_windows)
        return ns, self._added(parts, 1)

    def window_counts_to_stats(self, counts, samples):
        return self.subs[0].window_counts_to_stats(counts, samples)

    def window_stats_scale_exps(self):
        return self.subs[0].window_stats_scale_exps()

    def window_stats(self, counts=False):
        """-> (samples, J, D [nw, N-1, 8]) or (samples, int64 [nw, N-1, 16]): added over the shards as
        integers, then converted once"""
        ns, cnt = self.window_counts()
        if counts:
            return ns, cnt
        if not ns:
            raise RuntimeError("window statistics hold no sample")
        return (ns,) + self.window_counts_to_stats(cnt, ns)

    # lineage origin maps
    def lineage_origins_layout(self):
        """(leaves L, rows R, first local site of the first shard, sites over all shards)"""
        return self._layout_over_shards("lineage_origins_layout")

    def lineage_origin_rows(self):
        return self.subs[0].lineage_origin_rows()

    def lineage_origins_scale_exp(self):
        return self.subs[0].lineage_origins_scale_exp()

    def lineage_origins(self, counts=False):
        """-> (samples, rows [R, 2], origin [R, sites], age [L, sites]) over the group's owned sites, shards in
        genome order"""
        ns, parts = self._parts("lineage_origins", "lineage_origins", counts=True)
        origin, age = self._along_sites(parts, 2), self._along_sites(parts, 3)
        if counts:
            return ns, parts[0][1], origin, age
        k, d = self.lineage_origins_scale_exp(), float(ns) if ns else 1.0
        return ns, parts[0][1], origin / d, np.ldexp(age.astype(np.float64), -k) / d

    def lineage_origin_windows(self, W, first_window=0, n_windows=None):
        """-> (samples, uint64 [R, windows], uint64 [L, windows]): the shards' contributions to the windows of
        W global sites, added as integers"""
        W, n_windows = self._windows(W, first_window, n_windows)
        ns, parts = self._parts("lineage_origins", "lineage_origin_windows", W, first_window, n_windows)
        return ns, self._added(parts, 1, add_uint64), self._added(parts, 2, add_uint64)

    # domain size spectra: a shard's part is that of the sites it owns
    def domain_stats_layout(self):
        """(nodes N, bins, first local site of the first shard, sites over all shards, sites per block)"""
        return self._layout_over_shards("domain_stats_layout")

    def domain_stats_part(self):
        """-> (samples, hist, len_sum, edges): the shards' parts merged in genome order, unclosed"""
        ns, parts = self._parts("domain_stats", "domain_stats_part")
        return (ns,) + self._merged(parts, host.domain_parts_merge)

    def domain_stats(self):
        """-> (samples, hist [N, 2, 128], len_sum [N, 2]) over the group's owned sites, closed"""
        ns, hist, len_sum, edges = self.domain_stats_part()
        return (ns,) + host.domain_part_close(hist, len_sum, edges)

    # domain turnover: likewise
    def domain_turnover_layout(self):
        """(rows R, bins, first local site of the first shard, sites over all shards, sites per block)"""
        return self._layout_over_shards("domain_turnover_layout")

    def domain_turnover_part(self):
        """-> (samples, hist, len_sum, edges): the shards' parts merged in genome order, unclosed"""
        ns, parts = self._parts("domain_turnover", "domain_turnover_part")
        return (ns,) + self._merged(parts, host.turnover_parts_merge)

    def domain_turnover(self):
        """-> (samples, hist [R, 2, 2, 128], len_sum [R, 2, 2]) over the group's owned sites, closed"""
        ns, hist, len_sum, edges = self.domain_turnover_part()
        return (ns,) + host.turnover_part_close(hist, len_sum, edges)

    # spatial correlations: likewise
    def enable_spatial_correlation(self, max_lag, max_samples):
        self._corr_lag = int(max_lag)
        self._each_call("enable_spatial_correlation", max_lag, max_samples)

    def spatial_correlation_layout(self):
        """(rows R, max_lag, first local site of the first shard, sites over all shards, sites per block)"""
        return self._layout_over_shards("spatial_correlation_layout")

    def spatial_correlation_part(self):
        """-> (samples, sites, n11, edges): the shards' parts merged in genome order, unclosed"""
        ns, parts = self._parts("spatial_correlation", "spatial_correlation_part")
        return (ns,) + self._merged(parts, host.corr_parts_merge)

    def spatial_correlation(self):
        """-> (samples, n11, left1, right1), each [R, L + 1], over the group's owned sites, closed"""
        ns, cnt, n11, edges = self.spatial_correlation_part()
        return (ns,) + host.corr_part_close(cnt, n11, edges)

    # domain maps: a shard's part is that of the sites it owns
    def enable_domain_maps(self, sizes, state=1, max_samples=1 << 21):
        self._dmaps_on = bool(np.size(sizes))
        self._each_call("enable_domain_maps", sizes, state, max_samples)

    def domain_maps_layout(self):
        """(nodes N, sizes, state, first local site of the first shard, sites over all shards, sites per block)"""
        lay = self._each_call("domain_maps_layout")
        return lay[0][:4] + (sum(v[4] for v in lay),) + lay[0][5:]

    def domain_maps_part(self):
        """-> (samples, sites, counts, edges): the shards' parts merged in genome order"""
        ns, parts = self._parts("domain_maps", "domain_maps_part")
        sizes = self.subs[0].domain_maps_layout()[1]
        return (ns,) + self._merged(parts, lambda ps: host.domain_maps_merge(sizes, ps))

    def domain_maps(self, counts=False):
        """-> (samples, maps [N, K, sites]) over the group's owned sites"""
        ns, _, c, _ = self.domain_maps_part()
        return ns, _per_sample(c, ns, counts)

    # change tracts: a shard's part is that of the sites it owns
    def change_tracts_layout(self):
        """(branches B, classes, bins, first local site of the first shard, sites over all shards, sites per block)"""
        lay = self._each_call("change_tracts_layout")
        return lay[0][:4] + (sum(v[4] for v in lay),) + lay[0][5:]

    def change_tracts_part(self):
        """-> (samples, hist, len_sum, edges): the shards' parts merged in genome order, unclosed"""
        ns, parts = self._parts("change_tracts", "change_tracts_part")
        return (ns,) + self._merged(parts, host.tract_parts_merge)

    def change_tracts(self):
        """-> (samples, hist [B, 27, 128], len_sum [B, 27]) over the group's owned sites, closed"""
        ns, hist, len_sum, edges = self.change_tracts_part()
        return (ns,) + host.tract_part_close(hist, len_sum, edges)

    # chain mixing diagnostics: rows by site; the shards ran the same runs, so their pair counts agree
    def mixing_layout(self):
        """(first local site of the first shard, sites over all shards, max_lag)"""
        lay = self._each_call("mixing_layout")
        return lay[0][0], sum(v[1] for v in lay), lay[0][2]

    def _mixing_parts(self, name, *args):
        ns, parts = self._parts("mixing", name, *args)
        if any(p[1] != parts[0][1] for p in parts) or (
                name == "mixing" and any(not np.array_equal(p[2], parts[0][2]) for p in parts)):
            raise RuntimeError("the shards of the group hold mixing samples of different runs (their pair counts differ)")
        return ns, parts

    def mixing(self, counts=False):
        """-> DeviceSampler.mixing over the group's owned sites, shards in genome order"""
        ns, parts = self._mixing_parts("mixing", True)
        out = (ns, parts[0][1], parts[0][2], self._along_sites(parts, 3, axis=0), self._along_sites(parts, 4, axis=0),
               self._along_sites(parts, 5, axis=0), self._along_sites(parts, 6, axis=1))
        return out if counts else host.mixing_summary(*out)

    def mixing_windows(self, W, first_window=0, n_windows=None):
        """-> (samples, moved_pairs, uint64 [windows]): the shards' contributions to the windows of W global sites,
        added"""
        W, n_windows = self._windows(W, first_window, n_windows)
        ns, parts = self._mixing_parts("mixing_windows", W, first_window, n_windows)
        return ns, parts[0][1], self._added(parts, 2)

    # epoch statistics: every shard adds the triples centred at its owned sites
    def epoch_stats_layout(self):
        return self.subs[0].epoch_stats_layout()

    def epoch_raw(self):
        """-> (samples, uint64 [N-1, P, 32]): the shards' raw parts, added as integers"""
        ns, parts = self._parts("epoch_stats", "epoch_raw")
        return ns, self._added(parts, 1, host.epoch_raw_add)

    def epoch_stats(self, counts=False):
        """-> (samples, J, D [N-1, P, 8]) or the closed integers: added over the shards as integers, then
        closed once"""
        ns, raw = self.epoch_raw()
        _, k, fixT = self.epoch_stats_layout()
        return host.epoch_finish(raw, fixT, k, ns, counts)

    def counters(self):
        out = {}
        for s in self.subs:
            for key, v in s.counters().items():
                out[key] = out.get(key, 0) + v
        out["sweeps"] = self.subs[0].counters()["sweeps"]
        return out

    def set_timing(self, on):
        for s in self.subs:
            s.set_timing(on)

    def set_options(self, **kw):
        for s in self.subs:
            s.set_options(**kw)

    def set_direct_sampler(self, on=True, fused=False):
        for s in self.subs:
            s.set_direct_sampler(on, fused=fused)

    def phase_mode(self):
        """kernels of a colour phase (DeviceSampler.phase_mode) -- of the largest shard"""
        return min(s.phase_mode() for s in self.subs)

    def kernel_time_ms(self):
        """launch-weighted mean duration of the shards' colour-phase launches, and their number"""
        tot, n = 0.0, 0
        for s in self.subs:
            ms, nl = s.kernel_time_ms()
            tot += ms * nl
            n += nl
        return (tot / n if n else 0.0), n


def _enable_on_every_shard(name):
    """LocalGroup's enable_<stem>: DeviceSampler's, with its arguments, on every shard"""
    @functools.wraps(getattr(DeviceSampler, name))
    def method(self, *args, **kwargs):
        self._each_call(name, *args, **kwargs)
    return method


for _s in CHAIN:
    if "enable_" + _s.stem not in vars(LocalGroup):
        setattr(LocalGroup, "enable_" + _s.stem, _enable_on_every_shard("enable_" + _s.stem))
    setattr(LocalGroup, "reset_" + _s.stem, summary_method(LocalGroup._reset_summary, _s, "reset_" + _s.stem))
    setattr(LocalGroup, "accumulate_" + _s.stem,
            summary_method(LocalGroup._accumulate_summary, _s, "accumulate_" + _s.stem))
    setattr(LocalGroup, _s.stem + "_samples", summary_method(LocalGroup._summary_samples, _s, _s.stem + "_samples"))
