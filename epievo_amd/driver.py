"""ctypes face of libepv_driver.so (include/epievo_mi355x_driver.h): the C++ EM driver
epv::SingleSiteSampler -- the code path of the drop-in CLIs -- for bench.py and the tests.
Every GPU slot in this process (CppSampler(devices=[...])) or one slot per process
(CppSampler(rank=(device, world, rank, id)))."""
import ctypes as C

import numpy as np

from . import _build
from .host import FlatPaths
from . import host
from .summaries import _per_sample

_lib = None
vp, dp, u8p, u32p, u64p = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)

DRIVER_SYMBOLS = ["epvd_create", "epvd_unique_id", "epvd_create_rank", "epvd_destroy", "epvd_last_error", "epvd_shard_cuts",
                  "epvd_reset", "epvd_reset_model", "epvd_run_mcmc", "epvd_scale_jump_times", "epvd_download_sizes",
                  "epvd_download", "epvd_layout", "epvd_set_options", "epvd_set_timing", "epvd_kernel_time_ms",
                  "epvd_phase_mode", "epvd_set_unobserved", "epvd_set_leaf_evidence", "epvd_set_regions", "epvd_set_path_average", "epvd_path_average_sizes", "epvd_download_path_average",
                  "epvd_set_branch_events", "epvd_branch_events_sizes", "epvd_download_branch_events",
                  "epvd_download_branch_event_windows",
                  "epvd_set_window_stats", "epvd_window_stats_sizes", "epvd_download_window_stats",
                  "epvd_set_epoch_stats", "epvd_epoch_stats_sizes", "epvd_download_epoch_stats",
                  "epvd_set_lineage_origins", "epvd_reset_lineage_origins", "epvd_accumulate_lineage_origins",
                  "epvd_lineage_origin_rows", "epvd_lineage_origins_scale_exp", "epvd_lineage_origins_sizes", "epvd_download_lineage_origins",
                  "epvd_download_lineage_origin_windows",
                  "epvd_set_domain_stats", "epvd_reset_domain_stats", "epvd_accumulate_domain_stats",
                  "epvd_domain_part_sizes", "epvd_download_domain_part", "epvd_download_domain_stats",
                  "epvd_set_turnover", "epvd_reset_turnover", "epvd_accumulate_turnover",
                  "epvd_turnover_part_sizes", "epvd_download_turnover_part", "epvd_download_turnover",
                  "epvd_set_tracts", "epvd_reset_tracts", "epvd_accumulate_tracts",
                  "epvd_tracts_part_sizes", "epvd_download_tracts_part", "epvd_download_tracts",
                  "epvd_set_corr", "epvd_reset_corr", "epvd_accumulate_corr",
                  "epvd_corr_part_sizes", "epvd_download_corr_part", "epvd_download_corr",
                  "epvd_set_dmaps", "epvd_reset_dmaps", "epvd_accumulate_dmaps", "epvd_dmaps_sizes", "epvd_download_dmaps",
                  "epvd_set_change_patterns", "epvd_change_patterns_sizes", "epvd_download_change_patterns",
                  "epvd_download_change_pattern_windows",
                  "epvd_set_mixing", "epvd_mixing_sizes", "epvd_download_mixing"]


def lib():
    global _lib
    if _lib is None:
        _build.build_hip()
        _build.build_comm()
        L = C.CDLL(_build.build_driver())
        L.epvd_create.restype = vp
        L.epvd_create.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_int), C.c_uint32]
        L.epvd_unique_id.argtypes = [vp]
        L.epvd_create_rank.restype = vp
        L.epvd_create_rank.argtypes = [C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, vp, C.c_uint32]
        L.epvd_destroy.argtypes = [vp]
        L.epvd_last_error.restype = C.c_char_p
        L.epvd_last_error.argtypes = [vp]
        L.epvd_shard_cuts.argtypes = [C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, u64p]
        L.epvd_reset.argtypes = [vp, dp, dp, C.c_int, u32p, u32p, dp, C.c_uint64, u8p, u64p, dp, C.c_uint64]
        L.epvd_reset_model.argtypes = [vp, dp, dp]
        L.epvd_run_mcmc.argtypes = [vp, C.c_uint64, C.c_uint64, dp, dp, dp]
        L.epvd_scale_jump_times.argtypes = [vp, dp, C.c_int]
        L.epvd_download_sizes.argtypes = [vp, u64p, u64p]
        L.epvd_download.argtypes = [vp, u8p, u64p, dp]
        L.epvd_layout.argtypes = [vp, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), u64p]
        L.epvd_set_options.argtypes = [vp, C.c_uint32]
        L.epvd_set_timing.argtypes = [vp, C.c_int]
        L.epvd_kernel_time_ms.argtypes = [vp, dp, u64p]
        L.epvd_phase_mode.argtypes = [vp, u32p]
        L.epvd_set_unobserved.argtypes = [vp, C.c_uint64, C.c_int, u8p]
        L.epvd_set_leaf_evidence.argtypes = [vp, C.c_uint64, C.c_int, C.POINTER(C.c_float)]
        L.epvd_set_regions.argtypes = [vp, C.c_uint64, u64p]
        L.epvd_set_path_average.argtypes = [vp, C.c_uint32]
        L.epvd_path_average_sizes.argtypes = [vp, u64p, u32p, u64p]
        L.epvd_download_path_average.argtypes = [vp, u32p]
        L.epvd_set_branch_events.argtypes = [vp, C.c_int]
        L.epvd_branch_events_sizes.argtypes = [vp, u64p, u64p]
        L.epvd_download_branch_events.argtypes = [vp, u32p]
        L.epvd_download_branch_event_windows.argtypes = [vp, C.c_uint64, C.c_uint64, u64p, u64p]
        L.epvd_set_change_patterns.argtypes = [vp, C.c_int]
        L.epvd_change_patterns_sizes.argtypes = [vp, u64p, u32p, u64p]
        L.epvd_download_change_patterns.argtypes = [vp, u32p]
        L.epvd_download_change_pattern_windows.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, u64p, u64p]
        L.epvd_set_mixing.argtypes = [vp, C.c_uint32]
        L.epvd_mixing_sizes.argtypes = [vp, u64p, u32p]
        L.epvd_download_mixing.argtypes = [vp, u64p, u32p, u64p]
        L.epvd_set_window_stats.argtypes = [vp, C.c_uint64]
        L.epvd_window_stats_sizes.argtypes = [vp, u64p, u64p, u64p]
        L.epvd_download_window_stats.argtypes = [vp, C.POINTER(C.c_int64), dp, dp]
        L.epvd_set_epoch_stats.argtypes = [vp, C.c_uint32]
        L.epvd_epoch_stats_sizes.argtypes = [vp, C.POINTER(C.c_uint32), u64p]
        L.epvd_download_epoch_stats.argtypes = [vp, u64p, C.POINTER(C.c_int), u64p, dp, dp]
        ip = C.POINTER(C.c_int)
        L.epvd_set_lineage_origins.argtypes = [vp, C.c_int]
        L.epvd_reset_lineage_origins.argtypes = [vp]
        L.epvd_accumulate_lineage_origins.argtypes = [vp]
        L.epvd_lineage_origin_rows.argtypes = [vp, u32p, u32p, u32p, u32p]
        L.epvd_lineage_origins_scale_exp.argtypes = [vp, ip]
        L.epvd_lineage_origins_sizes.argtypes = [vp, u64p, u64p, ip, u64p]
        L.epvd_download_lineage_origins.argtypes = [vp, u32p, u64p]
        L.epvd_download_lineage_origin_windows.argtypes = [vp, C.c_uint64, C.c_uint64, u64p, u64p, ip, u64p]
        L.epvd_set_domain_stats.argtypes = [vp, C.c_uint64]
        L.epvd_reset_domain_stats.argtypes = [vp]
        L.epvd_accumulate_domain_stats.argtypes = [vp]
        L.epvd_domain_part_sizes.argtypes = [vp, u32p, u64p]
        L.epvd_download_domain_part.argtypes = [vp, u64p, u64p, u64p]
        L.epvd_download_domain_stats.argtypes = [vp, C.c_uint32, u64p, u64p, u64p]
        L.epvd_set_turnover.argtypes = [vp, C.c_uint64]
        L.epvd_reset_turnover.argtypes = [vp]
        L.epvd_accumulate_turnover.argtypes = [vp]
        L.epvd_turnover_part_sizes.argtypes = [vp, u32p, u64p]
        L.epvd_download_turnover_part.argtypes = [vp, u64p, u64p, u64p]
        L.epvd_download_turnover.argtypes = [vp, C.c_uint32, u64p, u64p, u64p]
        L.epvd_set_tracts.argtypes = [vp, C.c_uint64]
        L.epvd_reset_tracts.argtypes = [vp]
        L.epvd_accumulate_tracts.argtypes = [vp]
        L.epvd_tracts_part_sizes.argtypes = [vp, u32p, u64p]
        L.epvd_download_tracts_part.argtypes = [vp, u64p, u64p, u64p]
        L.epvd_download_tracts.argtypes = [vp, C.c_uint32, u64p, u64p, u64p]
        L.epvd_set_corr.argtypes = [vp, C.c_uint32, C.c_uint64]
        L.epvd_reset_corr.argtypes = [vp]
        L.epvd_accumulate_corr.argtypes = [vp]
        L.epvd_corr_part_sizes.argtypes = [vp, u32p, u32p, u64p, u64p]
        L.epvd_download_corr_part.argtypes = [vp, u64p, u64p]
        L.epvd_download_corr.argtypes = [vp, C.c_uint32, C.c_uint32, u64p, u64p, u64p, u64p]
        L.epvd_set_dmaps.argtypes = [vp, C.c_uint32, u32p, C.c_uint32, C.c_uint64]
        L.epvd_reset_dmaps.argtypes = [vp]
        L.epvd_accumulate_dmaps.argtypes = [vp]
        L.epvd_dmaps_sizes.argtypes = [vp, u32p, u32p, u64p, u64p]
        L.epvd_download_dmaps.argtypes = [vp, u32p, u64p]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class DriverError(RuntimeError):
    pass


def unique_id():
    """RCCL id for a one-slot-per-process run (rank 0 makes it, the launcher passes it around)"""
    buf = (C.c_uint8 * 128)()
    if lib().epvd_unique_id(buf) != 0:
        raise DriverError("epvd_unique_id failed")
    return bytes(buf)


def shard_cuts(n_sites, world, burn_in, batch):
    cuts = np.zeros(world + 1, np.uint64)
    g = lib().epvd_shard_cuts(n_sites, world, burn_in, batch, _p(cuts, C.c_uint64))
    return [int(x) for x in cuts[:g + 1]]


class CppSampler:
    def __init__(self, burn_in, batch, devices=(0,), capacity=0, rank=None):
        self.L = lib()
        self.burn_in, self.batch = int(burn_in), int(batch)
        if rank is None:
            devs = (C.c_int * len(devices))(*devices)
            self.h = self.L.epvd_create(self.burn_in, self.batch, len(devices), devs, capacity)
        else:
            device, world, r, ident = rank
            idb = (C.c_uint8 * 128).from_buffer_copy(ident)
            self.h = self.L.epvd_create_rank(self.burn_in, self.batch, device, world, r, idb, capacity)
        if not self.h:
            raise DriverError(self.L.epvd_last_error(None).decode())
        self.B = self.n_global = self.pattern_rows = 0
        self._options = 0          # the option word last handed to epvd_set_options

    def close(self):
        if getattr(self, "h", None):
            self.L.epvd_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _ck(self, rc):
        if rc != 0:
            raise DriverError(self.L.epvd_last_error(self.h).decode())

    def reset(self, model, tree=None, fp=None, n_global=0):
        rates = np.ascontiguousarray(model.rates, np.float64)
        T = np.ascontiguousarray(model.T, np.float64)
        if fp is None:
            self._ck(self.L.epvd_reset_model(self.h, _p(rates, C.c_double), _p(T, C.c_double)))
            return
        self.B, self.n_nodes = tree.n_nodes - 1, tree.n_nodes
        self.n_global = int(n_global) or fp.n_sites
        # rows of the change patterns: 12 + 2 (N-1) + internal non-root nodes
        self.pattern_rows = 12 + 2 * self.B + int((np.asarray(tree.subtree_sizes)[1:] > 1).sum())
        jumps = fp.jumps if len(fp.jumps) else np.zeros(1)
        self._ck(self.L.epvd_reset(self.h, _p(rates, C.c_double), _p(T, C.c_double), tree.n_nodes,
                                   _p(tree.parent_ids, C.c_uint32), _p(tree.subtree_sizes, C.c_uint32),
                                   _p(tree.branches, C.c_double), fp.n_sites, _p(fp.init, C.c_uint8),
                                   _p(fp.offsets, C.c_uint64), _p(jumps, C.c_double), n_global))

    def run_mcmc(self, seed, em_iteration=0):
        J, D, acc = np.zeros(self.B * 8), np.zeros(self.B * 8), C.c_double(0)
        self._ck(self.L.epvd_run_mcmc(self.h, seed, em_iteration, _p(J, C.c_double), _p(D, C.c_double), C.byref(acc)))
        return J, D, acc.value

    def scale_jump_times(self, branches):
        nb = np.ascontiguousarray(branches, np.float64)
        self._ck(self.L.epvd_scale_jump_times(self.h, _p(nb, C.c_double), len(nb)))

    def paths(self):
        n, tot = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epvd_download_sizes(self.h, C.byref(n), C.byref(tot)))
        E = self.B * n.value
        init, off, jumps = np.zeros(E, np.uint8), np.zeros(E + 1, np.uint64), np.zeros(max(tot.value, 1))
        self._ck(self.L.epvd_download(self.h, _p(init, C.c_uint8), _p(off, C.c_uint64), _p(jumps, C.c_double)))
        return FlatPaths(n.value, self.n_nodes, init, off, jumps[:tot.value])

    def layout(self):
        buf = C.create_string_buffer(512)
        ns, npart, rccl, halo = C.c_int(0), C.c_int(0), C.c_int(0), C.c_uint64(0)
        self._ck(self.L.epvd_layout(self.h, buf, 512, C.byref(ns), C.byref(npart), C.byref(rccl), C.byref(halo)))
        return {"text": buf.value.decode(), "slots_here": ns.value, "parts_here": npart.value,
                "rccl": bool(rccl.value), "halo": halo.value}

    def set_options(self, reference_proposal_ratio=False, forward_rejection=False, sample_root=False):
        """EPV_OPT_* of include/epievo_mi355x.h on every context, those of later resets included.  These three bits;
        EPV_OPT_DIRECT_SAMPLER and EPV_OPT_DIRECT_FUSED stay as set_direct_sampler left them and EPV_OPT_LEAF_FAST as
        set_leaf_fast did, so the order of the calls does not matter"""
        self._options = (1 if reference_proposal_ratio else 0) | (2 if forward_rejection else 0) | \
            (4 if sample_root else 0) | (self._options & (24 | 32))
        self._ck(self.L.epvd_set_options(self.h, self._options))

    def set_direct_sampler(self, on=True, fused=False):
        """EPV_OPT_DIRECT_SAMPLER (fused=True: and EPV_OPT_DIRECT_FUSED) on every context, those of later resets
        included: these bits of the word set_options last wrote, the others kept; on=False clears both"""
        self._options = (self._options & ~24) | ((8 | (16 if fused else 0)) if on else 0)
        self._ck(self.L.epvd_set_options(self.h, self._options))

    def set_leaf_fast(self, on=True):
        """EPV_OPT_LEAF_FAST on every context, those of later resets included: a held mask or table keeps the fused
        phase, the second or the third proposal kernel (leaf variants) instead of the first; this bit of the word,
        the others kept"""
        self._options = (self._options & ~32) | (32 if on else 0)
        self._ck(self.L.epvd_set_options(self.h, self._options))

    def set_timing(self, every):
        self._ck(self.L.epvd_set_timing(self.h, int(every)))

    def kernel_time_ms(self):
        a, k = C.c_double(0), C.c_uint64(0)
        self._ck(self.L.epvd_kernel_time_ms(self.h, C.byref(a), C.byref(k)))
        return a.value, k.value

    def phase_mode(self):
        m = C.c_uint32(0)
        self._ck(self.L.epvd_phase_mode(self.h, C.byref(m)))
        return m.value

    def set_unobserved(self, mask):
        """missing leaf data over the whole genome (epvd_set_unobserved): mask[b-1, s] != 0 -> the leaf end
        state of branch b at site s is resampled with the history.  Shape (n_nodes - 1, n_sites), or flat
        once reset() has set the tree; None clears.  Kept across reset(model), applied by every later
        reset(model, tree, paths)."""
        if mask is None:
            self._ck(self.L.epvd_set_unobserved(self.h, 0, 0, None))
            return
        m = np.asarray(mask)
        if m.ndim == 1:
            if not self.B:
                raise ValueError("a flat mask needs the tree: pass shape (n_nodes - 1, n_sites) before reset()")
            m = m.reshape(self.B, -1)
        m = np.ascontiguousarray(m != 0, np.uint8)
        self._ck(self.L.epvd_set_unobserved(self.h, m.shape[1], m.shape[0] + 1, _p(m, C.c_uint8)))

    def set_leaf_evidence(self, p_state1):
        """leaf evidence over the whole genome (epvd_set_leaf_evidence): p_state1[b-1, s] = P(the leaf end state
        of branch b at site s is 1 | that cell's own observation), float32, NaN = none.  Shape
        (n_nodes - 1, n_sites), or flat once reset() has set the tree; None clears.  Kept and applied as
        set_unobserved's mask is."""
        if p_state1 is None:
            self._ck(self.L.epvd_set_leaf_evidence(self.h, 0, 0, None))
            return
        r = np.asarray(p_state1, np.float32)
        if r.ndim == 1:
            if not self.B:
                raise ValueError("a flat table needs the tree: pass shape (n_nodes - 1, n_sites) before reset()")
            r = r.reshape(self.B, -1)
        r = np.ascontiguousarray(r)
        self._ck(self.L.epvd_set_leaf_evidence(self.h, r.shape[1], r.shape[0] + 1, _p(r, C.c_float)))

    def set_regions(self, lengths):
        """genomic regions of the whole genome (epvd_set_regions): their numbers of sites in its order, each at least
        3, summing to it (host.read_regions reads them from a file).  Their end sites are held fixed on every
        context, and run_mcmc's acceptance rate is over the sites that can be updated.  Kept and applied as
        set_unobserved's mask is; None clears."""
        if lengths is None:
            self._ck(self.L.epvd_set_regions(self.h, 0, None))
            return
        m = np.ascontiguousarray([int(x) for x in lengths], np.uint64)
        self._ck(self.L.epvd_set_regions(self.h, len(m), _p(m, C.c_uint64)))

    def enable_path_average(self, n_points):
        """the average history of the sampled paths on every context (0 = off); kept across reset()"""
        self._ck(self.L.epvd_set_path_average(self.h, int(n_points)))

    def path_average(self, counts=False):
        """-> (samples, [N-1, sites, P]) over the sites of this process: float64 averages or uint32 counts"""
        nv, P, ns = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        self._ck(self.L.epvd_path_average_sizes(self.h, C.byref(nv), C.byref(P), C.byref(ns)))
        out = np.zeros(max(nv.value, 1), np.uint32)
        self._ck(self.L.epvd_download_path_average(self.h, _p(out, C.c_uint32)))
        out = out[:nv.value].reshape(self.B, -1, P.value)
        ns = int(ns.value)
        return ns, _per_sample(out, ns, counts)

    def enable_branch_events(self, on=True):
        """posterior branch-event maps on every context (False = off); kept across reset()"""
        self._ck(self.L.epvd_set_branch_events(self.h, 1 if on else 0))

    def branch_events(self, counts=False):
        """-> (samples, [6, N-1, sites]) over the sites of this process: float64 counts / samples or uint32 counts"""
        nv, ns = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epvd_branch_events_sizes(self.h, C.byref(nv), C.byref(ns)))
        out = np.zeros(max(nv.value, 1), np.uint32)
        self._ck(self.L.epvd_download_branch_events(self.h, _p(out, C.c_uint32)))
        out = out[:nv.value].reshape(6, self.B, -1)
        ns = int(ns.value)
        return ns, _per_sample(out, ns, counts)

    def branch_event_windows(self, W):
        """-> (samples, uint64 [6, N-1, windows]): the planes summed over windows of W global sites (the
        contexts of this process added)"""
        W = int(W)
        if W < 1:
            raise ValueError("a window holds at least one site")
        nw = (self.n_global + W - 1) // W
        out, ns = np.zeros((6, self.B, nw), np.uint64), C.c_uint64(0)
        self._ck(self.L.epvd_download_branch_event_windows(self.h, W, nw, _p(out, C.c_uint64), C.byref(ns)))
        return int(ns.value), out

    def enable_mixing(self, max_lag=8):
        """chain mixing diagnostics on every context (0 = off); kept across reset()"""
        self._ck(self.L.epvd_set_mixing(self.h, int(max_lag)))

    def mixing(self, counts=False):
        """-> DeviceSampler.mixing over the sites of this process: the counts, or host.mixing_summary of them"""
        n, K = C.c_uint64(0), C.c_uint32(0)
        self._ck(self.L.epvd_mixing_sizes(self.h, C.byref(n), C.byref(K)))
        n, K = int(n.value), int(K.value)
        words, moved = np.zeros(K + 2, np.uint64), np.zeros(max(n, 1), np.uint32)
        sums = np.zeros(max((2 + K) * n, 1), np.uint64)
        self._ck(self.L.epvd_download_mixing(self.h, _p(words, C.c_uint64), _p(moved, C.c_uint32), _p(sums, C.c_uint64)))
        sums = sums[:(2 + K) * n].reshape(2 + K, n)
        pairs = np.concatenate([np.zeros(1, np.uint64), words[2:]])
        out = (int(words[0]), int(words[1]), pairs, moved[:n], sums[0], sums[1], sums[2:])
        return out if counts else host.mixing_summary(*out)

    def enable_change_patterns(self, on=True):
        """change patterns on every context (False = off); kept across reset()"""
        self._ck(self.L.epvd_set_change_patterns(self.h, 1 if on else 0))

    def change_patterns(self, counts=False):
        """-> (samples, [R, sites]) over the sites of this process: float64 counts / samples or uint32 counts"""
        nv, R, ns = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        self._ck(self.L.epvd_change_patterns_sizes(self.h, C.byref(nv), C.byref(R), C.byref(ns)))
        out = np.zeros(max(nv.value, 1), np.uint32)
        self._ck(self.L.epvd_download_change_patterns(self.h, _p(out, C.c_uint32)))
        out = out[:nv.value].reshape(R.value, -1)
        ns = int(ns.value)
        return ns, _per_sample(out, ns, counts)

    def change_pattern_windows(self, W):
        """-> (samples, uint64 [R, windows]): the rows summed over windows of W global sites (the slots and
        contexts of this process added)"""
        W = int(W)
        if W < 1:
            raise ValueError("a window holds at least one site")
        nw = (self.n_global + W - 1) // W
        out, ns = np.zeros((self.pattern_rows, nw), np.uint64), C.c_uint64(0)
        self._ck(self.L.epvd_download_change_pattern_windows(self.h, W, self.pattern_rows, nw, _p(out, C.c_uint64),
                                                             C.byref(ns)))
        return int(ns.value), out

    def enable_window_stats(self, W):
        """regional sufficient statistics on every context: J and D per window of W global sites (0 = off);
        kept across reset()"""
        self._ck(self.L.epvd_set_window_stats(self.h, int(W)))

    def window_stats(self, counts=False):
        """-> (samples, J, D [windows, N-1, 8]) per sample, or (samples, int64 [windows, N-1, 16]): the slots
        and contexts of this process added as integers"""
        W, nw, ns = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epvd_window_stats_sizes(self.h, C.byref(W), C.byref(nw), C.byref(ns)))
        cnt = np.zeros((nw.value, self.B, 16), np.int64)
        J, D = np.zeros((nw.value, self.B, 8)), np.zeros((nw.value, self.B, 8))
        self._ck(self.L.epvd_download_window_stats(self.h, _p(cnt, C.c_int64), _p(J, C.c_double), _p(D, C.c_double)))
        ns = int(ns.value)
        if counts:
            return ns, cnt
        if not ns:
            raise DriverError("window statistics hold no sample")
        return ns, J, D

    def enable_epoch_stats(self, P):
        """epoch statistics on every context: J and D per branch and epoch, P epochs per branch (0 = off);
        kept across reset()"""
        self._ck(self.L.epvd_set_epoch_stats(self.h, int(P)))

    def epoch_stats(self, counts=False):
        """-> (samples, J, D [N-1, P, 8]) per sample, or with counts=True the closed integers (samples, J int64,
        D Python ints in an object array): the slots and contexts of this process added as integers"""
        P, ns = C.c_uint32(0), C.c_uint64(0)
        self._ck(self.L.epvd_epoch_stats_sizes(self.h, C.byref(P), C.byref(ns)))
        closed = np.zeros((self.B, P.value, 24), np.uint64)
        k, f = np.zeros(max(self.B, 1), np.intc), np.zeros(max(self.B, 1), np.uint64)
        J, D = np.zeros((self.B, P.value, 8)), np.zeros((self.B, P.value, 8))
        self._ck(self.L.epvd_download_epoch_stats(self.h, _p(closed, C.c_uint64), _p(k, C.c_int), _p(f, C.c_uint64),
                                                  _p(J, C.c_double), _p(D, C.c_double)))
        ns = int(ns.value)
        if counts:
            return ns, closed[..., :8].astype(np.int64), \
                closed[..., 8:16].astype(object) + closed[..., 16:24].astype(object) * (1 << 64)
        if not ns:
            raise DriverError("epoch statistics hold no sample")
        return ns, J, D

    def enable_lineage_origins(self, on=True):
        """lineage origin maps on every context (False = off); kept across reset()"""
        self._ck(self.L.epvd_set_lineage_origins(self.h, 1 if on else 0))

    def reset_lineage_origins(self):
        self._ck(self.L.epvd_reset_lineage_origins(self.h))

    def accumulate_lineage_origins(self):
        self._ck(self.L.epvd_accumulate_lineage_origins(self.h))

    def lineage_origin_rows(self):
        """uint32 [R, 2]: per row the leaf node and the branch node (0 = the leaf's root row)"""
        nl, nr = C.c_uint32(0), C.c_uint32(0)
        self._ck(self.L.epvd_lineage_origin_rows(self.h, C.byref(nl), C.byref(nr), None, None))
        leaf, node = np.zeros(max(nr.value, 1), np.uint32), np.zeros(max(nr.value, 1), np.uint32)
        self._ck(self.L.epvd_lineage_origin_rows(self.h, C.byref(nl), C.byref(nr), _p(leaf, C.c_uint32),
                                                 _p(node, C.c_uint32)))
        return np.stack([leaf[:nr.value], node[:nr.value]], axis=1)

    def lineage_origins(self, counts=False):
        """-> (samples, rows [R, 2], origin [R, sites], age [L, sites]) over the sites of this process: origin /
        samples and age * 2^-k / samples, or the uint32 and uint64 sums"""
        rows = self.lineage_origin_rows()
        R, L = len(rows), int((rows[:, 1] == 0).sum())
        no, na, k, ns = C.c_uint64(0), C.c_uint64(0), C.c_int(0), C.c_uint64(0)
        self._ck(self.L.epvd_lineage_origins_sizes(self.h, C.byref(no), C.byref(na), C.byref(k), C.byref(ns)))
        origin, age = np.zeros(max(no.value, 1), np.uint32), np.zeros(max(na.value, 1), np.uint64)
        self._ck(self.L.epvd_download_lineage_origins(self.h, _p(origin, C.c_uint32), _p(age, C.c_uint64)))
        origin, age, ns = origin[:no.value].reshape(R, -1), age[:na.value].reshape(L, -1), int(ns.value)
        if counts:
            return ns, rows, origin, age
        d = float(ns) if ns else 1.0
        return ns, rows, origin / d, np.ldexp(age.astype(np.float64), -k.value) / d

    def lineage_origins_scale_exp(self):
        """k: an age integer is a time in units of 2^-k"""
        k = C.c_int(0)
        self._ck(self.L.epvd_lineage_origins_scale_exp(self.h, C.byref(k)))
        return int(k.value)

    def lineage_origin_windows(self, W):
        """-> (samples, uint64 [R, windows], uint64 [L, windows]): the origin rows and the ages summed over windows
        of W global sites (the slots and contexts of this process added)"""
        W = int(W)
        if W < 1:
            raise ValueError("a window holds at least one site")
        rows = self.lineage_origin_rows()
        nw = (self.n_global + W - 1) // W
        o = np.zeros((len(rows), nw), np.uint64)
        a = np.zeros((int((rows[:, 1] == 0).sum()), nw), np.uint64)
        ns = C.c_uint64(0)
        self._ck(self.L.epvd_download_lineage_origin_windows(self.h, W, nw, _p(o, C.c_uint64), _p(a, C.c_uint64), None,
                                                             C.byref(ns)))
        return int(ns.value), o, a

    def enable_domain_stats(self, max_samples):
        """domain size spectra on every context, for at most max_samples samples (0 = off); kept across reset()"""
        self._ck(self.L.epvd_set_domain_stats(self.h, int(max_samples)))

    def reset_domain_stats(self):
        self._ck(self.L.epvd_reset_domain_stats(self.h))

    def accumulate_domain_stats(self):
        self._ck(self.L.epvd_accumulate_domain_stats(self.h))

    def domain_stats_part(self):
        """-> (samples, hist [N, 2, 128], len_sum [N, 2], edges [samples, N, 2]), uint64: the parts of the slots and
        contexts of this process merged in genome order, unclosed"""
        N, ns = C.c_uint32(0), C.c_uint64(0)
        self._ck(self.L.epvd_domain_part_sizes(self.h, C.byref(N), C.byref(ns)))
        N, ns = int(N.value), int(ns.value)
        hist, len_sum = np.zeros((max(N, 1), 2, 128), np.uint64), np.zeros((max(N, 1), 2), np.uint64)
        edges = np.zeros((max(ns, 1), max(N, 1), 2), np.uint64)
        self._ck(self.L.epvd_download_domain_part(self.h, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64),
                                                  _p(edges.reshape(-1)[:max(ns * N * 2, 1)], C.c_uint64)))
        return ns, hist[:N], len_sum[:N], edges.reshape(-1)[:ns * N * 2].reshape(ns, N, 2)

    def domain_stats(self):
        """-> (samples, hist [N, 2, 128], len_sum [N, 2]): the closed result over the genome (one slot per process:
        an error; merge the processes' domain_stats_part with host.domain_parts_merge, then host.domain_part_close)"""
        N = self.B + 1
        hist, len_sum, ns = np.zeros((N, 2, 128), np.uint64), np.zeros((N, 2), np.uint64), C.c_uint64(0)
        self._ck(self.L.epvd_download_domain_stats(self.h, N, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64), C.byref(ns)))
        return int(ns.value), hist, len_sum

    def enable_domain_turnover(self, max_samples):
        """domain turnover on every context, for at most max_samples samples (0 = off); kept across reset()"""
        self._ck(self.L.epvd_set_turnover(self.h, int(max_samples)))

    def reset_domain_turnover(self):
        self._ck(self.L.epvd_reset_turnover(self.h))

    def accumulate_domain_turnover(self):
        self._ck(self.L.epvd_accumulate_turnover(self.h))

    def domain_turnover_part(self):
        """-> (samples, hist [R, 2, 2, 128], len_sum [R, 2, 2], edges [samples, R, 2]), uint64: the parts of the slots
        and contexts of this process merged in genome order, unclosed"""
        R, ns = C.c_uint32(0), C.c_uint64(0)
        self._ck(self.L.epvd_turnover_part_sizes(self.h, C.byref(R), C.byref(ns)))
        R, ns = int(R.value), int(ns.value)
        hist, len_sum = np.zeros((max(R, 1), 2, 2, 128), np.uint64), np.zeros((max(R, 1), 2, 2), np.uint64)
        edges = np.zeros((max(ns, 1), max(R, 1), 2), np.uint64)
        self._ck(self.L.epvd_download_turnover_part(self.h, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64),
                                                    _p(edges.reshape(-1)[:max(ns * R * 2, 1)], C.c_uint64)))
        return ns, hist[:R], len_sum[:R], edges.reshape(-1)[:ns * R * 2].reshape(ns, R, 2)

    def domain_turnover(self):
        """-> (samples, hist [R, 2, 2, 128], len_sum [R, 2, 2]): the closed result over the genome (one slot per
        process: an error; merge the processes' domain_turnover_part with host.turnover_parts_merge, then
        host.turnover_part_close)"""
        R = 2 * self.B
        hist, len_sum, ns = np.zeros((R, 2, 2, 128), np.uint64), np.zeros((R, 2, 2), np.uint64), C.c_uint64(0)
        self._ck(self.L.epvd_download_turnover(self.h, R, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64), C.byref(ns)))
        return int(ns.value), hist, len_sum

    def enable_change_tracts(self, max_samples):
        """change tracts on every context, for at most max_samples samples (0 = off); kept across reset()"""
        self._ck(self.L.epvd_set_tracts(self.h, int(max_samples)))

    def reset_change_tracts(self):
        self._ck(self.L.epvd_reset_tracts(self.h))

    def accumulate_change_tracts(self):
        self._ck(self.L.epvd_accumulate_tracts(self.h))

    def change_tracts_part(self):
        """-> (samples, hist [B, 27, 128], len_sum [B, 27], edges [samples, B, 2]), uint64: the parts of the slots and
        contexts of this process merged in genome order, unclosed"""
        B, ns = C.c_uint32(0), C.c_uint64(0)
        self._ck(self.L.epvd_tracts_part_sizes(self.h, C.byref(B), C.byref(ns)))
        B, ns = int(B.value), int(ns.value)
        hist, len_sum = np.zeros((max(B, 1), 27, 128), np.uint64), np.zeros((max(B, 1), 27), np.uint64)
        edges = np.zeros((max(ns, 1), max(B, 1), 2), np.uint64)
        self._ck(self.L.epvd_download_tracts_part(self.h, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64),
                                                  _p(edges.reshape(-1)[:max(ns * B * 2, 1)], C.c_uint64)))
        return ns, hist[:B], len_sum[:B], edges.reshape(-1)[:ns * B * 2].reshape(ns, B, 2)

    def change_tracts(self):
        """-> (samples, hist [B, 27, 128], len_sum [B, 27]): the closed result over the genome (one slot per process:
        an error; merge the processes' change_tracts_part with host.tract_parts_merge, then host.tract_part_close)"""
        B = self.B
        hist, len_sum, ns = np.zeros((B, 27, 128), np.uint64), np.zeros((B, 27), np.uint64), C.c_uint64(0)
        self._ck(self.L.epvd_download_tracts(self.h, B, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64), C.byref(ns)))
        return int(ns.value), hist, len_sum

    def enable_domain_maps(self, sizes, state=1, max_samples=1 << 21):
        """domain maps on every context (DeviceSampler.enable_domain_maps; an empty list: off)"""
        z = host.domain_map_sizes(sizes) if np.size(sizes) else np.zeros(0, np.uint32)
        self._ck(self.L.epvd_set_dmaps(self.h, len(z), _p(z if len(z) else np.zeros(1, np.uint32), C.c_uint32), int(state),
                                       int(max_samples)))
        self._dmaps_sizes = tuple(int(L) for L in z)

    def reset_domain_maps(self):
        self._ck(self.L.epvd_reset_dmaps(self.h))

    def accumulate_domain_maps(self):
        self._ck(self.L.epvd_accumulate_dmaps(self.h))

    def domain_maps_part(self):
        """-> (samples, sites, counts uint32 [N, K, sites], edges uint64 [samples, N, 2, EW]): the parts of this
        process's slots and contexts merged in genome order"""
        N, K, ns, cnt = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epvd_dmaps_sizes(self.h, C.byref(N), C.byref(K), C.byref(ns), C.byref(cnt)))
        N, K, ns, cnt = int(N.value), int(K.value), int(ns.value), int(cnt.value)
        EW = (2 * (self._dmaps_sizes[-1] - 1) + 63) // 64
        counts = np.zeros(max(N * K * cnt, 1), np.uint32)
        edges = np.zeros(max(ns * N * 2 * EW, 1), np.uint64)
        self._ck(self.L.epvd_download_dmaps(self.h, _p(counts, C.c_uint32), _p(edges, C.c_uint64)))
        return ns, cnt, counts[:N * K * cnt].reshape(N, K, cnt), edges[:ns * N * 2 * EW].reshape(ns, N, 2, EW)

    def domain_maps(self, counts=False):
        """-> (samples, maps [N, K, sites]) over the sites of this process (DeviceSampler.domain_maps)"""
        ns, _, c, _ = self.domain_maps_part()
        return ns, _per_sample(c, ns, counts)

    def enable_spatial_correlation(self, max_lag, max_samples):
        """spatial correlations on every context, lags 0 .. max_lag, for at most max_samples samples (max_lag = 0:
        off); kept across reset()"""
        self._ck(self.L.epvd_set_corr(self.h, int(max_lag), int(max_samples)))
        self._corr_lag = int(max_lag)

    def reset_spatial_correlation(self):
        self._ck(self.L.epvd_reset_corr(self.h))

    def accumulate_spatial_correlation(self):
        self._ck(self.L.epvd_accumulate_corr(self.h))

    def spatial_correlation_part(self):
        """-> (samples, sites, n11 [R, L + 1], edges [samples, R, 2, ceil(L / 64)]), uint64: the parts of the slots
        and contexts of this process merged in genome order, unclosed"""
        R, L, ns, cnt = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epvd_corr_part_sizes(self.h, C.byref(R), C.byref(L), C.byref(ns), C.byref(cnt)))
        R, L, ns = int(R.value), int(L.value), int(ns.value)
        LW = (L + 63) // 64
        n11 = np.zeros(max(R * (L + 1), 1), np.uint64)
        edges = np.zeros(max(ns * R * 2 * LW, 1), np.uint64)
        self._ck(self.L.epvd_download_corr_part(self.h, _p(n11, C.c_uint64), _p(edges, C.c_uint64)))
        return ns, int(cnt.value), n11[:R * (L + 1)].reshape(R, L + 1), edges[:ns * R * 2 * LW].reshape(ns, R, 2, LW)

    def spatial_correlation(self):
        """-> (samples, n11, left1, right1), each [R, L + 1]: the closed result over the genome (one slot per process:
        an error; merge the processes' spatial_correlation_part with host.corr_parts_merge, then
        host.corr_part_close)"""
        R, L = 2 * self.B + 1, getattr(self, "_corr_lag", 0)
        n11, left1, right1 = (np.zeros((R, L + 1), np.uint64) for _ in range(3))
        ns = C.c_uint64(0)
        self._ck(self.L.epvd_download_corr(self.h, R, L, _p(n11, C.c_uint64), _p(left1, C.c_uint64),
                                           _p(right1, C.c_uint64), C.byref(ns)))
        return int(ns.value), n11, left1, right1
