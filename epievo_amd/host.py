"""ctypes binding of libepv_host.so -- the C++ host library (model, M-step, file
formats, synthetic-input simulator).  No GPU code, no oracle code."""
import ctypes as C
import os

import numpy as np

from . import _build

_lib = None


def lib():
    global _lib
    if _lib is None:
        path = _build.HOST_SO
        if not os.path.exists(path):
            _build.build_host()
        L = C.CDLL(path)
        dp, u8p, u32p, u64p = (C.POINTER(C.c_double), C.POINTER(C.c_uint8),
                               C.POINTER(C.c_uint32), C.POINTER(C.c_uint64))
        L.epvh_last_error.restype = C.c_char_p
        L.epvh_model_read.argtypes = [C.c_char_p, C.c_int, dp, dp, dp]
        L.epvh_rate_scaling_factor.argtypes = [dp]
        L.epvh_rate_scaling_factor.restype = C.c_double
        L.epvh_m_step.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, C.c_char_p, C.c_int]
        L.epvh_simulate.argtypes = [dp, dp, C.c_int, u32p, dp, C.c_uint64, C.c_uint64]
        L.epvh_simulate.restype = C.c_void_p
        L.epvh_paths_total_jumps.argtypes = [C.c_void_p]
        L.epvh_paths_total_jumps.restype = C.c_uint64
        L.epvh_paths_n_sites.argtypes = [C.c_void_p]
        L.epvh_paths_n_sites.restype = C.c_uint64
        L.epvh_paths_n_nodes.argtypes = [C.c_void_p]
        L.epvh_paths_copy.argtypes = [C.c_void_p, u8p, u64p, dp]
        L.epvh_paths_free.argtypes = [C.c_void_p]
        L.epvh_read_paths.argtypes = [C.c_char_p, C.c_char_p, C.c_int, dp, C.c_int]
        L.epvh_read_paths.restype = C.c_void_p
        L.epvh_write_paths.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint64, dp, u8p, u64p, dp]
        L.epvh_read_tree.argtypes = [C.c_char_p, C.c_int, u32p, u32p, dp, C.c_char_p, C.c_int]
        L.epvh_indep_m_step.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp]
        L.epvh_model_from_indep_rates.argtypes = [dp, dp, dp, dp]
        L.epvh_initialize_paths_heuristic.argtypes = [C.c_uint64, C.c_int, u32p, u32p, dp, C.c_uint64, u8p]
        L.epvh_initialize_paths_heuristic.restype = C.c_void_p
        i64p, ip = C.POINTER(C.c_int64), C.POINTER(C.c_int)
        L.epvh_regional_rate_factors.argtypes = [C.c_int, C.c_uint64, dp, dp, dp, dp]
        L.epvh_regional_rate_factors.restype = None
        L.epvh_collapsed_log_likelihood.argtypes = [C.c_int, dp, dp, dp]
        L.epvh_collapsed_log_likelihood.restype = C.c_double
        L.epvh_write_window_stats.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_uint64, C.c_uint64, dp, ip, i64p,
                                              C.c_uint64, dp, dp, dp]
        L.epvh_read_window_stats.argtypes = [C.c_char_p]
        L.epvh_read_window_stats.restype = C.c_void_p
        L.epvh_window_stats_dims.argtypes = [C.c_void_p, u64p, u64p, u64p, u64p, u64p]
        L.epvh_window_stats_dims.restype = None
        L.epvh_window_stats_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_int, dp, ip, i64p, i64p, dp, dp]
        L.epvh_window_stats_copy.restype = None
        L.epvh_window_stats_free.argtypes = [C.c_void_p]
        L.epvh_window_stats_free.restype = None
        L.epvh_write_lineage_origins.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, u32p, u32p, C.c_uint64, C.c_uint64,
                                                 C.c_int, u64p, u64p, C.c_uint64]
        L.epvh_read_lineage_origins.argtypes = [C.c_char_p]
        L.epvh_read_lineage_origins.restype = C.c_void_p
        L.epvh_lineage_origins_dims.argtypes = [C.c_void_p, u64p, u64p, u64p, ip, u64p, u64p, u64p]
        L.epvh_lineage_origins_dims.restype = None
        L.epvh_lineage_origins_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_int, u64p, u64p]
        L.epvh_lineage_origins_copy.restype = None
        L.epvh_lineage_origins_free.argtypes = [C.c_void_p]
        L.epvh_lineage_origins_free.restype = None
        u64pp = C.POINTER(u64p)
        L.epvh_domain_bin.argtypes = [C.c_uint64]
        L.epvh_domain_bin.restype = C.c_uint32
        L.epvh_domain_bin_range.argtypes = [C.c_uint32, u64p, u64p]
        L.epvh_domain_bin_range.restype = None
        L.epvh_domain_parts_merge.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, u64pp, u64pp, u64pp, u64p, u64p, u64p]
        L.epvh_domain_part_close.argtypes = [C.c_uint32, C.c_uint64, u64p, u64p, u64p]
        L.epvh_write_domain_stats.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, u64p, u64p]
        L.epvh_read_domain_stats.argtypes = [C.c_char_p]
        L.epvh_read_domain_stats.restype = C.c_void_p
        L.epvh_domain_stats_dims.argtypes = [C.c_void_p, u64p, u64p, u64p]
        L.epvh_domain_stats_dims.restype = None
        L.epvh_domain_stats_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_int, u64p, u64p]
        L.epvh_domain_stats_copy.restype = None
        L.epvh_domain_stats_free.argtypes = [C.c_void_p]
        L.epvh_domain_stats_free.restype = None
        L.epvh_turnover_parts_merge.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, u64pp, u64pp, u64pp, u64p, u64p, u64p]
        L.epvh_turnover_part_close.argtypes = [C.c_uint32, C.c_uint64, u64p, u64p, u64p]
        L.epvh_write_domain_turnover.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, u64p, u64p]
        L.epvh_read_domain_turnover.argtypes = [C.c_char_p]
        L.epvh_read_domain_turnover.restype = C.c_void_p
        L.epvh_domain_turnover_dims.argtypes = [C.c_void_p, u64p, u64p, u64p]
        L.epvh_domain_turnover_dims.restype = None
        L.epvh_domain_turnover_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_int, u64p, u64p]
        L.epvh_domain_turnover_copy.restype = None
        L.epvh_domain_turnover_free.argtypes = [C.c_void_p]
        L.epvh_domain_turnover_free.restype = None
        L.epvh_tract_parts_merge.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, u64pp, u64pp, u64pp, u64p, u64p, u64p]
        L.epvh_tract_part_close.argtypes = [C.c_uint32, C.c_uint64, u64p, u64p, u64p]
        L.epvh_write_change_tracts.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, u64p, u64p]
        L.epvh_read_change_tracts.argtypes = [C.c_char_p]
        L.epvh_read_change_tracts.restype = C.c_void_p
        L.epvh_change_tracts_dims.argtypes = [C.c_void_p, u64p, u64p, u64p]
        L.epvh_change_tracts_dims.restype = None
        L.epvh_change_tracts_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_int, u64p, u64p]
        L.epvh_change_tracts_copy.restype = None
        L.epvh_change_tracts_free.argtypes = [C.c_void_p]
        L.epvh_change_tracts_free.restype = None
        L.epvh_corr_parts_merge.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, u64p, u64pp, u64pp, u64p, u64p,
                                            u64p]
        L.epvh_corr_part_close.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, u64p, u64p, u64p, u64p]
        L.epvh_write_spatial_correlation.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint32, u64p, u64p,
                                                     u64p]
        L.epvh_read_spatial_correlation.argtypes = [C.c_char_p]
        L.epvh_read_spatial_correlation.restype = C.c_void_p
        L.epvh_spatial_correlation_dims.argtypes = [C.c_void_p, u64p, u64p, u64p, u64p, u64p]
        L.epvh_spatial_correlation_dims.restype = None
        L.epvh_spatial_correlation_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_int, u64p, u64p, u64p]
        L.epvh_spatial_correlation_copy.restype = None
        L.epvh_spatial_correlation_free.argtypes = [C.c_void_p]
        L.epvh_spatial_correlation_free.restype = None
        u32pp = C.POINTER(u32p)
        L.epvh_domain_map_members.argtypes = [u64p, C.c_uint64, C.c_uint32, u64p]
        L.epvh_domain_maps_part.argtypes = [C.c_uint32, C.c_uint32, u32p, C.c_uint64, u64p, u32p, u64p]
        L.epvh_domain_maps_merge.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, u32p, C.c_uint64, u64p, u32pp, u64pp,
                                             u32p, u64p, u64p]
        L.epvh_write_domain_maps.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, u32p, C.c_uint64,
                                             C.c_uint64, u64p]
        L.epvh_read_domain_maps.argtypes = [C.c_char_p]
        L.epvh_read_domain_maps.restype = C.c_void_p
        L.epvh_domain_maps_dims.argtypes = [C.c_void_p, u64p]
        L.epvh_domain_maps_dims.restype = None
        L.epvh_domain_maps_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_int, u32p, u64p]
        L.epvh_domain_maps_copy.restype = None
        L.epvh_domain_maps_free.argtypes = [C.c_void_p]
        L.epvh_domain_maps_free.restype = None
        u64p_, u32 = C.POINTER(C.c_uint64), C.c_uint32
        L.epvh_epoch_edges.argtypes = [C.c_uint64, u32, u64p_]
        L.epvh_epoch_edges.restype = None
        L.epvh_epoch_close.argtypes = [u64p_, u64p_, u32, u32, u64p_]
        L.epvh_epoch_counts_to_stats.argtypes = [u64p_, C.POINTER(C.c_int), u32, u32, C.c_uint64, dp, dp]
        L.epvh_write_epoch_stats.argtypes = [C.c_char_p, C.c_char_p, C.c_int, u32, dp, C.POINTER(C.c_int), u64p_, u64p_,
                                             C.c_uint64, dp]
        L.epvh_read_epoch_stats.argtypes = [C.c_char_p]
        L.epvh_read_epoch_stats.restype = C.c_void_p
        L.epvh_epoch_stats_dims.argtypes = [C.c_void_p, u64p_, u64p_, u64p_, u64p_]
        L.epvh_epoch_stats_dims.restype = None
        L.epvh_epoch_stats_copy.argtypes = [C.c_void_p, C.c_char_p, C.c_int, dp, C.POINTER(C.c_int), u64p_, dp, dp]
        L.epvh_epoch_stats_copy.restype = None
        L.epvh_epoch_stats_free.argtypes = [C.c_void_p]
        L.epvh_epoch_stats_free.restype = None
        L.epvh_phase_plan.argtypes = [C.c_int, u32p, u32p, C.c_uint64, u32, C.c_double, u32, C.c_uint64, C.c_uint64,
                                      C.POINTER(C.c_char_p), C.c_int, C.POINTER(u32)]
        L.epvh_phase_plan2.argtypes = L.epvh_phase_plan.argtypes + [u64p_]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Model:
    """rates[8], T[4] (row-major 2x2), baseline[4]"""

    def __init__(self, rates, T, baseline):
        self.rates = np.ascontiguousarray(rates, dtype=np.float64)
        self.T = np.ascontiguousarray(T, dtype=np.float64)
        self.baseline = np.ascontiguousarray(baseline, dtype=np.float64)

    @staticmethod
    def read(param_file, scale=True):
        rates, T, bl = np.zeros(8), np.zeros(4), np.zeros(4)
        if lib().epvh_model_read(param_file.encode(), int(scale), _p(rates, C.c_double),
                                 _p(T, C.c_double), _p(bl, C.c_double)):
            raise RuntimeError(lib().epvh_last_error().decode())
        return Model(rates, T, bl)


class Tree:
    def __init__(self, subtree_sizes, parent_ids, branches, node_names=None):
        self.subtree_sizes = np.ascontiguousarray(subtree_sizes, dtype=np.uint32)
        self.parent_ids = np.ascontiguousarray(parent_ids, dtype=np.uint32)
        self.branches = np.ascontiguousarray(branches, dtype=np.float64)
        self.n_nodes = len(self.subtree_sizes)
        self.node_names = node_names or ["node_%d" % i for i in range(self.n_nodes)]

    @staticmethod
    def read(tree_file, max_nodes=4096):
        st, pa, br = (np.zeros(max_nodes, np.uint32), np.zeros(max_nodes, np.uint32),
                      np.zeros(max_nodes))
        buf = C.create_string_buffer(64 * max_nodes)
        n = lib().epvh_read_tree(tree_file.encode(), max_nodes, _p(st, C.c_uint32),
                                 _p(pa, C.c_uint32), _p(br, C.c_double), buf, len(buf))
        if n < 0:
            raise RuntimeError(lib().epvh_last_error().decode())
        return Tree(st[:n].copy(), pa[:n].copy(), br[:n].copy(), buf.value.decode().split("\n"))

    @staticmethod
    def single_branch(evo_time):
        return Tree([2, 1], [0, 0], [0.0, evo_time], ["root", "leaf"])

    @staticmethod
    def balanced(n_leaves, branch_len):
        """synthetic balanced binary tree in pre-order (BASELINE config 5)"""
        sizes, parents, br = [], [], []

        def rec(leaves, parent):
            me = len(sizes)
            sizes.append(1)
            parents.append(parent)
            br.append(0.0 if parent < 0 else branch_len)
            if leaves > 1:
                rec(leaves // 2, me)
                rec(leaves - leaves // 2, me)
                sizes[me] = len(sizes) - me
        rec(n_leaves, -1)
        parents[0] = 0
        return Tree(sizes, parents, br)


class FlatPaths:
    """node-major flat local paths: entry (b-1)*n_sites + site, b = 1..n_nodes-1"""

    def __init__(self, n_sites, n_nodes, init, offsets, jumps):
        self.n_sites, self.n_nodes = int(n_sites), int(n_nodes)
        self.init = np.ascontiguousarray(init, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.jumps = np.ascontiguousarray(jumps, dtype=np.float64)

    @staticmethod
    def _from_handle(h):
        L = lib()
        n, N, tot = L.epvh_paths_n_sites(h), L.epvh_paths_n_nodes(h), L.epvh_paths_total_jumps(h)
        init = np.zeros((N - 1) * n, np.uint8)
        off = np.zeros((N - 1) * n + 1, np.uint64)
        jumps = np.zeros(max(tot, 1), np.float64)
        L.epvh_paths_copy(h, _p(init, C.c_uint8), _p(off, C.c_uint64), _p(jumps, C.c_double))
        L.epvh_paths_free(h)
        return FlatPaths(n, N, init, off, jumps[:tot])

    def counts(self):
        return np.diff(self.offsets).astype(np.int64)

    def slice_sites(self, lo, hi):
        """sub-range of sites [lo, hi) as a new FlatPaths"""
        n, B = self.n_sites, self.n_nodes - 1
        cnt = self.counts().reshape(B, n)[:, lo:hi]
        init = self.init.reshape(B, n)[:, lo:hi]
        offs = self.offsets[:-1].reshape(B, n)[:, lo:hi]
        pieces = [self.jumps[int(offs[b, 0]):int(offs[b, -1] + cnt[b, -1])] for b in range(B)]
        new_off = np.zeros(B * (hi - lo) + 1, np.uint64)
        new_off[1:] = np.cumsum(cnt.reshape(-1))
        return FlatPaths(hi - lo, self.n_nodes, init.reshape(-1).copy(), new_off,
                         np.concatenate(pieces) if pieces else np.zeros(0))


PLAN_PROPOSE = ("V1", "V2", "V3", "fused")
PLAN_JUMPS = ("fused", "segments", "jumps_all", "jumps")
PLAN_ACCEPT = ("fused", "accept3", "accept_cache", "accept_no_cache")


def plan_fields(w):
    """a plan word (EPV_PLAN_* of include/epievo_mi355x.h) as a dict of its fields"""
    return dict(word=w, propose=PLAN_PROPOSE[w & 3], gpool=bool(w >> 2 & 1), refq=bool(w >> 3 & 1),
                small_nn=w >> 4 & 15, p3_words=w >> 8 & 3, p3_slab_pool=bool(w >> 10 & 1),
                jumps=PLAN_JUMPS[w >> 12 & 3], accept=PLAN_ACCEPT[w >> 14 & 3], listed=bool(w >> 16 & 1),
                unobs=bool(w >> 17 & 1), evidence=bool(w >> 18 & 1), direct=bool(w >> 23 & 1),
                fused_lanes=(1 << (w >> 20 & 7)) if (w & 3) == 3 else 0)


def phase_plan(tree, n_sites, capacity, kbar, options=0, unobs_cells=0, evidence_cells=0, knobs={}):
    """the kernel variants of a colour phase, decided without a GPU by the code the device library decides with
    (csrc/epv_plan.h): what DeviceSampler.phase_plan() returns in a context with this tree, n_sites local sites of
    jump capacity `capacity` and a mean of kbar jumps per (site, branch), the option word `options` (EPV_OPT_*),
    so many unobserved and evidence leaf cells, and `knobs` (EPV_* names to values) as its environment"""
    return phase_plan_p2(tree, n_sites, capacity, kbar, options, unobs_cells, evidence_cells, knobs)[0]


def phase_plan_p2(tree, n_sites, capacity, kbar, options=0, unobs_cells=0, evidence_cells=0, knobs={}):
    """phase_plan, and beside it the launch shape of the second proposal kernel and of the fused phase in its
    buffers (plan_p2 of csrc/epv_plan.h): planned, fused, pool (LDS doubles per wave), lds (dynamic LDS bytes of
    the launch), fused_lanes"""
    names = [("%s=%s" % kv).encode() for kv in knobs.items()]
    arr = (C.c_char_p * max(len(names), 1))(*names)
    w = C.c_uint32(0)
    p2 = (C.c_uint64 * 5)()
    if lib().epvh_phase_plan2(tree.n_nodes, _p(tree.parent_ids, C.c_uint32), _p(tree.subtree_sizes, C.c_uint32),
                              int(n_sites), int(capacity), float(kbar), int(options), int(unobs_cells),
                              int(evidence_cells), arr, len(names), C.byref(w), p2):
        raise RuntimeError(lib().epvh_last_error().decode())
    return plan_fields(int(w.value)), dict(planned=bool(p2[0]), fused=bool(p2[1]), pool=int(p2[2]), lds=int(p2[3]),
                                           fused_lanes=int(p2[4]))


def simulate(model, tree, n_sites, seed):
    h = lib().epvh_simulate(_p(model.rates, C.c_double), _p(model.T, C.c_double), tree.n_nodes,
                            _p(tree.parent_ids, C.c_uint32), _p(tree.branches, C.c_double),
                            int(n_sites), int(seed))
    if not h:
        raise RuntimeError(lib().epvh_last_error().decode())
    return FlatPaths._from_handle(h)


def read_paths(path_file, max_nodes=4096):
    buf = C.create_string_buffer(64 * max_nodes)
    tt = np.zeros(max_nodes)
    h = lib().epvh_read_paths(path_file.encode(), buf, len(buf), _p(tt, C.c_double), max_nodes)
    if not h:
        raise RuntimeError(lib().epvh_last_error().decode())
    fp = FlatPaths._from_handle(h)
    return fp, buf.value.decode().split("\n"), tt[:fp.n_nodes].copy()


def write_paths(path_file, node_names, tot_times, fp):
    tt = np.ascontiguousarray(tot_times, dtype=np.float64)
    jumps = fp.jumps if len(fp.jumps) else np.zeros(1)
    if lib().epvh_write_paths(path_file.encode(), "\n".join(node_names).encode(), fp.n_nodes,
                              fp.n_sites, _p(tt, C.c_double), _p(fp.init, C.c_uint8),
                              _p(fp.offsets, C.c_uint64), _p(jumps, C.c_double)):
        raise RuntimeError(lib().epvh_last_error().decode())


def read_regions(path, n_sites):
    """the regions file of a genome (the chrom.sizes shape): one line per region, `name <whitespace> n_sites`, in the
    order of the paths file; a line that starts with # is a comment, an empty line is skipped.  Every region holds at
    least 3 sites and the lengths sum to n_sites.  -> the list of lengths.  A violation raises ValueError naming the
    line (the regions are the chromosomes, or the gap-free stretches of them, of SingleSiteSampler.set_regions)"""
    lengths, total, last = [], 0, 0
    with open(path) as f:
        for no, line in enumerate(f, 1):
            fields = line.split()
            if not fields or fields[0].startswith("#"):
                continue
            where = "%s, line %d" % (path, no)
            if len(fields) != 2:
                raise ValueError("%s: a region is `name n_sites`, found %d fields" % (where, len(fields)))
            try:
                m = int(fields[1])
            except ValueError:
                raise ValueError("%s: the number of sites of region %s is not an integer: %s"
                                 % (where, fields[0], fields[1])) from None
            if m < 3:
                raise ValueError("%s: region %s holds %d sites, a region holds at least 3" % (where, fields[0], m))
            total += m
            if total > n_sites:
                raise ValueError("%s: the regions up to %s hold %d sites, the paths hold %d"
                                 % (where, fields[0], total, n_sites))
            lengths.append(m)
            last = no
    if total != n_sites:
        raise ValueError("%s, line %d: the regions hold %d sites in all, the paths hold %d"
                         % (path, last, total, n_sites))
    return lengths


def region_fixed_mask(n_sites, lengths):
    """uint8 [n_sites]: 1 at the first and the last site of every region (DeviceSampler.set_fixed_sites).  A region
    of 3 sites has one site that is updated; two adjacent regions put two fixed sites side by side"""
    lengths = [int(m) for m in lengths]
    for k, m in enumerate(lengths):
        if m < 3:
            raise ValueError("region %d holds %d sites, a region holds at least 3" % (k, m))
    if sum(lengths) != int(n_sites):
        raise ValueError("the regions hold %d sites in all, the paths hold %d" % (sum(lengths), int(n_sites)))
    mask = np.zeros(int(n_sites), np.uint8)
    ends = np.cumsum(lengths)
    mask[ends - np.asarray(lengths)] = 1
    mask[ends - 1] = 1
    return mask


def m_step(model, tree_branches, J, D, optimize_branches=False):
    """The EM driver's M-step (est_params_histories.cpp:253-263).  Returns
    (new Model, new branches, llh, param-file text)."""
    n_nodes = len(tree_branches)
    rates, T, bl = model.rates.copy(), np.zeros(4), np.zeros(4)
    br = np.ascontiguousarray(tree_branches, dtype=np.float64).copy()
    J = np.ascontiguousarray(J, dtype=np.float64)
    D = np.ascontiguousarray(D, dtype=np.float64)
    llh = C.c_double(0.0)
    buf = C.create_string_buffer(512)
    if lib().epvh_m_step(int(optimize_branches), n_nodes, _p(J, C.c_double), _p(D, C.c_double),
                         _p(rates, C.c_double), _p(T, C.c_double), _p(bl, C.c_double),
                         _p(br, C.c_double), C.byref(llh), buf, len(buf)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return Model(rates, T, bl), br, llh.value, buf.value.decode()


def indep_m_step(rates, branches, J, D, optimize_branches=False):
    """M-step of the site-independent model (IndepSite.cpp:299-360) -> (rates[2], branches)"""
    r = np.ascontiguousarray(rates, np.float64).copy()
    br = np.ascontiguousarray(branches, np.float64).copy()
    J = np.ascontiguousarray(J, np.float64)
    D = np.ascontiguousarray(D, np.float64)
    if lib().epvh_indep_m_step(int(optimize_branches), len(br), _p(J, C.c_double), _p(D, C.c_double),
                               _p(r, C.c_double), _p(br, C.c_double)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return r, br


def model_from_indep_rates(rates2):
    r2 = np.ascontiguousarray(rates2, np.float64)
    rates, T, bl = np.zeros(8), np.zeros(4), np.zeros(4)
    if lib().epvh_model_from_indep_rates(_p(r2, C.c_double), _p(rates, C.c_double), _p(T, C.c_double),
                                         _p(bl, C.c_double)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return Model(rates, T, bl)


def initialize_paths_heuristic(seed, tree, states):
    """epievo_initialization's heuristic start; states [n_nodes][n_sites] uint8 (leaves filled,
    internal nodes overwritten) -> FlatPaths"""
    st = np.ascontiguousarray(states, np.uint8)
    h = lib().epvh_initialize_paths_heuristic(int(seed), tree.n_nodes, _p(tree.subtree_sizes, C.c_uint32),
                                              _p(tree.parent_ids, C.c_uint32), _p(tree.branches, C.c_double),
                                              st.shape[1], _p(st, C.c_uint8))
    if not h:
        raise RuntimeError(lib().epvh_last_error().decode())
    states[...] = st
    return FlatPaths._from_handle(h)


# ---- regional sufficient statistics (J and D per genomic window)
def regional_rate_factors(J, D, rates):
    """J, D [windows, N-1, 8] -> rho[windows] = sum J / sum D_c rate_c: per window the multiplier of the
    fitted rates that maximises log_likelihood(J, D, rho * rates); NaN where a window has no dwell time"""
    J = np.ascontiguousarray(J, np.float64)
    D = np.ascontiguousarray(D, np.float64)
    r = np.ascontiguousarray(rates, np.float64)
    if J.ndim != 3 or J.shape != D.shape or J.shape[2] != 8 or r.shape != (8,):
        raise ValueError("J and D are [windows, N-1, 8], rates [8]")
    out = np.zeros(J.shape[0])
    lib().epvh_regional_rate_factors(J.shape[1] + 1, J.shape[0], _p(J, C.c_double), _p(D, C.c_double),
                                     _p(r, C.c_double), _p(out, C.c_double))
    return out


def collapsed_log_likelihood(J, D, rates):
    """J, D [N-1, 8]: sum_c Jc log(rate_c) - Dc rate_c over the branches' sums (the M-step's objective)"""
    J = np.ascontiguousarray(J, np.float64)
    D = np.ascontiguousarray(D, np.float64)
    r = np.ascontiguousarray(rates, np.float64)
    return float(lib().epvh_collapsed_log_likelihood(J.shape[0] + 1, _p(J, C.c_double), _p(D, C.c_double),
                                                     _p(r, C.c_double)))


def write_window_stats(path, node_names, branches, scale_exp, window, samples, counts, J, D, rates):
    """the file of epievo_est_histories -r.  node_names, branches, scale_exp: per node, the root first;
    counts int64 [windows, N-1, 16]; J, D [windows, N-1, 8] per sample"""
    counts = np.ascontiguousarray(counts, np.int64)
    J = np.ascontiguousarray(J, np.float64)
    D = np.ascontiguousarray(D, np.float64)
    br = np.ascontiguousarray(branches, np.float64)
    k = np.ascontiguousarray(scale_exp, np.intc)
    r = np.ascontiguousarray(rates, np.float64)
    if lib().epvh_write_window_stats(path.encode(), "\n".join(node_names).encode(), len(br), counts.shape[0], int(window),
                                     _p(br, C.c_double), _p(k, C.c_int), _p(counts, C.c_int64), int(samples),
                                     _p(J, C.c_double), _p(D, C.c_double), _p(r, C.c_double)):
        raise RuntimeError(lib().epvh_last_error().decode())


def read_window_stats(path):
    """-> dict(samples, window, node_names, branches, scale_exp (non-root nodes), counts [windows, N-1, 16],
    all_J int64 [windows, 8], all_D [windows, 8], factor [windows])"""
    L = lib()
    h = L.epvh_read_window_stats(path.encode())
    if not h:
        raise RuntimeError(L.epvh_last_error().decode())
    try:
        ns, W, nw, B, nl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.epvh_window_stats_dims(h, C.byref(ns), C.byref(W), C.byref(nw), C.byref(B), C.byref(nl))
        nw, B = int(nw.value), int(B.value)
        buf = C.create_string_buffer(int(nl.value))        # the names as the file has them, however long
        br, k = np.zeros(max(B, 1)), np.zeros(max(B, 1), np.intc)
        counts = np.zeros((nw, B, 16), np.int64)
        aJ, aD, f = np.zeros((nw, 8), np.int64), np.zeros((nw, 8)), np.zeros(nw)
        L.epvh_window_stats_copy(h, buf, len(buf), _p(br, C.c_double), _p(k, C.c_int), _p(counts, C.c_int64),
                                 _p(aJ, C.c_int64), _p(aD, C.c_double), _p(f, C.c_double))
        return dict(samples=int(ns.value), window=int(W.value), node_names=buf.value.decode().split("\n"),
                    branches=br[:B], scale_exp=k[:B], counts=counts, all_J=aJ, all_D=aD, factor=f)
    finally:
        L.epvh_window_stats_free(h)


# ---- lineage origin maps (where each leaf's state arose, and how old it is)
def write_lineage_origins(path, node_names, rows, window, samples, scale_exp, origin, age):
    """the file of epievo_est_histories -O.  node_names: per node, the root first; rows uint32 [R, 2] (leaf node,
    branch node or 0); origin uint64 [R, windows] and age uint64 [L, windows]: integer window sums"""
    rows = np.asarray(rows, np.uint32).reshape(-1, 2)
    leaf, node = np.ascontiguousarray(rows[:, 0]), np.ascontiguousarray(rows[:, 1])
    origin = np.ascontiguousarray(origin, np.uint64)
    age = np.ascontiguousarray(age, np.uint64)
    if origin.ndim != 2 or age.ndim != 2 or origin.shape[0] != len(rows) or age.shape[1] != origin.shape[1] or \
            age.shape[0] != int((node == 0).sum()):
        raise ValueError("origin is [rows, windows], age [leaves, windows]")
    if lib().epvh_write_lineage_origins(path.encode(), "\n".join(node_names).encode(), len(rows), _p(leaf, C.c_uint32),
                                        _p(node, C.c_uint32), origin.shape[1], int(window), int(scale_exp),
                                        _p(origin, C.c_uint64), _p(age, C.c_uint64), int(samples)):
        raise RuntimeError(lib().epvh_last_error().decode())


def read_lineage_origins(path):
    """-> dict(samples, window, scale_exp, row_leaf, row_node (names per row; a root row names the root),
    origin uint64 [R, windows], age uint64 [L, windows])"""
    L = lib()
    h = L.epvh_read_lineage_origins(path.encode())
    if not h:
        raise RuntimeError(L.epvh_last_error().decode())
    try:
        ns, W, nw, R, nl, ln = (C.c_uint64(0) for _ in range(6))
        k = C.c_int(0)
        L.epvh_lineage_origins_dims(h, C.byref(ns), C.byref(W), C.byref(nw), C.byref(k), C.byref(R), C.byref(nl), C.byref(ln))
        R, nl, nw = int(R.value), int(nl.value), int(nw.value)
        b1, b2 = C.create_string_buffer(int(ln.value)), C.create_string_buffer(int(ln.value))
        origin, age = np.zeros((R, nw), np.uint64), np.zeros((nl, nw), np.uint64)
        o, a = (origin, age) if R * nw else (np.zeros(1, np.uint64), np.zeros(1, np.uint64))
        L.epvh_lineage_origins_copy(h, b1, b2, len(b1), _p(o, C.c_uint64), _p(a, C.c_uint64))
        return dict(samples=int(ns.value), window=int(W.value), scale_exp=int(k.value),
                    row_leaf=b1.value.decode().split("\n") if R else [],
                    row_node=b2.value.decode().split("\n") if R else [], origin=origin, age=age)
    finally:
        L.epvh_lineage_origins_free(h)


# ---- domain size spectra (run lengths of every node's state along the genome)
DOMAIN_BINS = 128


def domain_bin(length):
    """the bin of a run of `length` sites: the length itself below 16, then four bins per octave"""
    return int(lib().epvh_domain_bin(int(length)))


def domain_bin_range(b):
    """(lo, hi): the run lengths bin b holds, both included; (0, 0) for bin 0, which is never used"""
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    lib().epvh_domain_bin_range(int(b), C.byref(lo), C.byref(hi))
    return int(lo.value), int(hi.value)


def domain_bin_edges():
    """uint64 [128, 2]: per bin the smallest and the largest run length it holds"""
    return np.array([domain_bin_range(b) for b in range(DOMAIN_BINS)], np.uint64)


def _ptrs(arrays):
    return (C.POINTER(C.c_uint64) * len(arrays))(*[_p(a, C.c_uint64) for a in arrays])


def domain_parts_merge(parts):
    """parts: [(hist [N, 2, 128], len_sum [N, 2], edges [samples, N, 2])] of adjacent stretches of sites in genome
    order, of the same samples -> the part of their union (uint64 arrays of the same shapes)"""
    if not parts:
        raise ValueError("no parts")
    hists = [np.ascontiguousarray(p[0], np.uint64) for p in parts]
    sums = [np.ascontiguousarray(p[1], np.uint64) for p in parts]
    edges = [np.ascontiguousarray(p[2], np.uint64) for p in parts]
    N, ns = hists[0].shape[0], edges[0].shape[0]
    for h, l, e in zip(hists, sums, edges):
        if h.shape != (N, 2, DOMAIN_BINS) or l.shape != (N, 2) or e.shape != (ns, N, 2):
            raise ValueError("a part is hist [N, 2, 128], len_sum [N, 2], edges [samples, N, 2] of the same N and samples")
    hist, len_sum = np.zeros((N, 2, DOMAIN_BINS), np.uint64), np.zeros((N, 2), np.uint64)
    out = np.zeros((ns, N, 2), np.uint64)
    o = out if out.size else np.zeros(1, np.uint64)
    if lib().epvh_domain_parts_merge(len(parts), N, ns, _ptrs(hists), _ptrs(sums),
                                     _ptrs([e if e.size else np.zeros(1, np.uint64) for e in edges]),
                                     _p(hist, C.c_uint64), _p(len_sum, C.c_uint64), _p(o, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return hist, len_sum, out


def domain_part_close(hist, len_sum, edges):
    """a part -> the result (hist [N, 2, 128], len_sum [N, 2]): its first and last records are binned and added, a
    whole record once.  The runs at the two ends count with the length the stretch leaves them"""
    hist, len_sum = np.array(hist, np.uint64), np.array(len_sum, np.uint64)
    edges = np.ascontiguousarray(edges, np.uint64)
    N, ns = hist.shape[0], edges.shape[0]
    if hist.shape != (N, 2, DOMAIN_BINS) or len_sum.shape != (N, 2) or edges.shape != (ns, N, 2):
        raise ValueError("a part is hist [N, 2, 128], len_sum [N, 2], edges [samples, N, 2]")
    e = edges if edges.size else np.zeros(1, np.uint64)
    if lib().epvh_domain_part_close(N, ns, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64), _p(e, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return hist, len_sum


def domain_summary(samples, hist, len_sum):
    """-> (runs per sample [N, 2], mean run length [N, 2]) per node and state of a closed result; nan where a state
    has no run"""
    runs = np.asarray(hist, np.uint64).sum(axis=2, dtype=np.uint64).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return runs / float(samples), np.asarray(len_sum, np.uint64).astype(np.float64) / runs


def write_domain_stats(path, node_names, samples, hist, len_sum):
    """the file of epievo_est_histories -d: the closed result, integers only"""
    hist, len_sum = np.ascontiguousarray(hist, np.uint64), np.ascontiguousarray(len_sum, np.uint64)
    N = len(node_names)
    if hist.shape != (N, 2, DOMAIN_BINS) or len_sum.shape != (N, 2):
        raise ValueError("hist is [nodes, 2, 128], len_sum [nodes, 2]")
    if lib().epvh_write_domain_stats(path.encode(), "\n".join(node_names).encode(), int(samples), _p(hist, C.c_uint64),
                                     _p(len_sum, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())


def read_domain_stats(path):
    """-> dict(samples, node_names, hist uint64 [N, 2, 128], len_sum uint64 [N, 2])"""
    L = lib()
    h = L.epvh_read_domain_stats(path.encode())
    if not h:
        raise RuntimeError(L.epvh_last_error().decode())
    try:
        ns, N, ln = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.epvh_domain_stats_dims(h, C.byref(ns), C.byref(N), C.byref(ln))
        N = int(N.value)
        buf = C.create_string_buffer(int(ln.value))
        hist, len_sum = np.zeros((N, 2, DOMAIN_BINS), np.uint64), np.zeros((N, 2), np.uint64)
        a, b = (hist, len_sum) if N else (np.zeros(1, np.uint64), np.zeros(1, np.uint64))
        L.epvh_domain_stats_copy(h, buf, len(buf), _p(a, C.c_uint64), _p(b, C.c_uint64))
        return dict(samples=int(ns.value), node_names=buf.value.decode().split("\n") if N else [], hist=hist,
                    len_sum=len_sum)
    finally:
        L.epvh_domain_stats_free(h)


# ---- domain turnover (per branch, the runs of its start and end rows, kept or turned over)
def turnover_parts_merge(parts):
    """parts: [(hist [R, 2, 2, 128], len_sum [R, 2, 2], edges [samples, R, 2])] of adjacent stretches of sites in
    genome order, of the same samples -> the part of their union (uint64 arrays of the same shapes)"""
    if not parts:
        raise ValueError("no parts")
    hists = [np.ascontiguousarray(p[0], np.uint64) for p in parts]
    sums = [np.ascontiguousarray(p[1], np.uint64) for p in parts]
    edges = [np.ascontiguousarray(p[2], np.uint64) for p in parts]
    R, ns = hists[0].shape[0], edges[0].shape[0]
    for h, l, e in zip(hists, sums, edges):
        if h.shape != (R, 2, 2, DOMAIN_BINS) or l.shape != (R, 2, 2) or e.shape != (ns, R, 2):
            raise ValueError("a part is hist [R, 2, 2, 128], len_sum [R, 2, 2], edges [samples, R, 2] of the same R "
                             "and samples")
    hist, len_sum = np.zeros((R, 2, 2, DOMAIN_BINS), np.uint64), np.zeros((R, 2, 2), np.uint64)
    out = np.zeros((ns, R, 2), np.uint64)
    o = out if out.size else np.zeros(1, np.uint64)
    if lib().epvh_turnover_parts_merge(len(parts), R, ns, _ptrs(hists), _ptrs(sums),
                                       _ptrs([e if e.size else np.zeros(1, np.uint64) for e in edges]),
                                       _p(hist, C.c_uint64), _p(len_sum, C.c_uint64), _p(o, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return hist, len_sum, out


def turnover_part_close(hist, len_sum, edges):
    """a part -> the result (hist [R, 2, 2, 128], len_sum [R, 2, 2]): its first and last records are binned and
    added, a whole record once.  The runs at the two ends count with the length the stretch leaves them"""
    hist, len_sum = np.array(hist, np.uint64), np.array(len_sum, np.uint64)
    edges = np.ascontiguousarray(edges, np.uint64)
    R, ns = hist.shape[0], edges.shape[0]
    if hist.shape != (R, 2, 2, DOMAIN_BINS) or len_sum.shape != (R, 2, 2) or edges.shape != (ns, R, 2):
        raise ValueError("a part is hist [R, 2, 2, 128], len_sum [R, 2, 2], edges [samples, R, 2]")
    e = edges if edges.size else np.zeros(1, np.uint64)
    h, l = (hist, len_sum) if R else (np.zeros(1, np.uint64), np.zeros(1, np.uint64))
    if lib().epvh_turnover_part_close(R, ns, _p(h, C.c_uint64), _p(l, C.c_uint64), _p(e, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return hist, len_sum


def domain_turnover_summary(samples, hist, len_sum, tree):
    """a closed result -> dict of float64 [B] arrays, per branch b (child node b + 1): born, died, merged (parent
    gaps filled) and split (gaps opened) = turned-over runs per sample; born_size, died_size, merged_size,
    split_size = their mean lengths (nan where a class has no run); parent_domains and child_domains = the
    state-1 runs of the start and the end row per sample, kept or not"""
    hist, len_sum = np.asarray(hist, np.uint64), np.asarray(len_sum, np.uint64)
    B = tree.n_nodes - 1
    if hist.shape != (2 * B, 2, 2, DOMAIN_BINS) or len_sum.shape != (2 * B, 2, 2):
        raise ValueError("hist is [2 B, 2, 2, 128], len_sum [2 B, 2, 2] of the tree's B branches")
    runs = hist.sum(axis=3, dtype=np.uint64).astype(np.float64).reshape(B, 2, 2, 2)   # [b, row, state, kept]
    sites = len_sum.astype(np.float64).reshape(B, 2, 2, 2)
    ns = float(samples)
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for name, row, state in (("born", 1, 1), ("died", 0, 1), ("merged", 0, 0), ("split", 1, 0)):
            out[name] = runs[:, row, state, 0] / ns
            out[name + "_size"] = sites[:, row, state, 0] / runs[:, row, state, 0]
        out["parent_domains"] = runs[:, 0, 1, :].sum(axis=1) / ns
        out["child_domains"] = runs[:, 1, 1, :].sum(axis=1) / ns
    return out


def write_domain_turnover(path, branch_names, samples, hist, len_sum):
    """the file of epievo_est_histories -R: the closed result, integers only; branch_names = the child node's name
    of every branch"""
    hist, len_sum = np.ascontiguousarray(hist, np.uint64), np.ascontiguousarray(len_sum, np.uint64)
    B = len(branch_names)
    if hist.shape != (2 * B, 2, 2, DOMAIN_BINS) or len_sum.shape != (2 * B, 2, 2):
        raise ValueError("hist is [2 branches, 2, 2, 128], len_sum [2 branches, 2, 2]")
    if lib().epvh_write_domain_turnover(path.encode(), "\n".join(branch_names).encode(), int(samples),
                                        _p(hist, C.c_uint64), _p(len_sum, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())


def read_domain_turnover(path):
    """-> dict(samples, branch_names, hist uint64 [2 B, 2, 2, 128], len_sum uint64 [2 B, 2, 2])"""
    L = lib()
    h = L.epvh_read_domain_turnover(path.encode())
    if not h:
        raise RuntimeError(L.epvh_last_error().decode())
    try:
        ns, B, ln = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.epvh_domain_turnover_dims(h, C.byref(ns), C.byref(B), C.byref(ln))
        B = int(B.value)
        buf = C.create_string_buffer(int(ln.value))
        hist, len_sum = np.zeros((2 * B, 2, 2, DOMAIN_BINS), np.uint64), np.zeros((2 * B, 2, 2), np.uint64)
        a, b = (hist, len_sum) if B else (np.zeros(1, np.uint64), np.zeros(1, np.uint64))
        L.epvh_domain_turnover_copy(h, buf, len(buf), _p(a, C.c_uint64), _p(b, C.c_uint64))
        return dict(samples=int(ns.value), branch_names=buf.value.decode().split("\n") if B else [], hist=hist,
                    len_sum=len_sum)
    finally:
        L.epvh_domain_turnover_free(h)


# ---- change tracts (per branch, the maximal runs of changed sites by direction and flanks)
TRACT_CLASSES = 27     # EPV_TRACT_CLASSES: direction * 9 + left * 3 + right; direction gain, loss, mixed; flank 0, 1, none
TRACT_DIRECTIONS = ("gain", "loss", "mixed")


def tract_parts_merge(parts):
    """parts: [(hist [B, 27, 128], len_sum [B, 27], edges [samples, B, 2])] of adjacent stretches of sites in genome
    order, of the same samples -> the part of their union (uint64 arrays of the same shapes)"""
    if not parts:
        raise ValueError("no parts")
    hists = [np.ascontiguousarray(p[0], np.uint64) for p in parts]
    sums = [np.ascontiguousarray(p[1], np.uint64) for p in parts]
    edges = [np.ascontiguousarray(p[2], np.uint64) for p in parts]
    B, ns = hists[0].shape[0], edges[0].shape[0]
    for h, l, e in zip(hists, sums, edges):
        if h.shape != (B, TRACT_CLASSES, DOMAIN_BINS) or l.shape != (B, TRACT_CLASSES) or e.shape != (ns, B, 2):
            raise ValueError("a part is hist [B, 27, 128], len_sum [B, 27], edges [samples, B, 2] of the same B and "
                             "samples")
    hist, len_sum = np.zeros((B, TRACT_CLASSES, DOMAIN_BINS), np.uint64), np.zeros((B, TRACT_CLASSES), np.uint64)
    out = np.zeros((ns, B, 2), np.uint64)
    o = out if out.size else np.zeros(1, np.uint64)
    if lib().epvh_tract_parts_merge(len(parts), B, ns, _ptrs(hists), _ptrs(sums),
                                    _ptrs([e if e.size else np.zeros(1, np.uint64) for e in edges]),
                                    _p(hist, C.c_uint64), _p(len_sum, C.c_uint64), _p(o, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return hist, len_sum, out


def tract_part_close(hist, len_sum, edges):
    """a part -> the result (hist [B, 27, 128], len_sum [B, 27]): the tracts still open at the two ends are binned
    with flank 2 (none), a whole record once"""
    hist, len_sum = np.array(hist, np.uint64), np.array(len_sum, np.uint64)
    edges = np.ascontiguousarray(edges, np.uint64)
    B, ns = hist.shape[0], edges.shape[0]
    if hist.shape != (B, TRACT_CLASSES, DOMAIN_BINS) or len_sum.shape != (B, TRACT_CLASSES) or edges.shape != (ns, B, 2):
        raise ValueError("a part is hist [B, 27, 128], len_sum [B, 27], edges [samples, B, 2]")
    e = edges if edges.size else np.zeros(1, np.uint64)
    h, l = (hist, len_sum) if B else (np.zeros(1, np.uint64), np.zeros(1, np.uint64))
    if lib().epvh_tract_part_close(B, ns, _p(h, C.c_uint64), _p(l, C.c_uint64), _p(e, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return hist, len_sum


# the events of change_tract_summary: name -> (direction, left flank, right flank).  A gained tract left of a kept
# domain (flanks 0 | 1) grew that domain at its left edge; a lost tract with flanks 0 | 1 took the left edge of the
# domain to its right
TRACT_EVENTS = {"born": (0, 0, 0), "filled": (0, 1, 1), "grew_left": (0, 0, 1), "grew_right": (0, 1, 0),
                "died": (1, 0, 0), "split": (1, 1, 1), "shrank_left": (1, 0, 1), "shrank_right": (1, 1, 0)}


def change_tract_summary(samples, hist, len_sum, tree):
    """a closed result -> dict of float64 [B] arrays, per branch b (child node b + 1) and per sample: born, died,
    filled, split (gain or loss between flanks 0 | 0 or 1 | 1), grew_left, grew_right, shrank_left, shrank_right (the
    edge of the kept domain that moved), mixed (both directions in one tract, both flanks present) and open (a tract
    at a genome end, any direction); <name>_size = the mean length of each (nan where there is none); and
    net_edge_sites = the sites per sample that kept domains gained at their edges: grew sites - shrank sites"""
    hist, len_sum = np.asarray(hist, np.uint64), np.asarray(len_sum, np.uint64)
    B = tree.n_nodes - 1
    if hist.shape != (B, TRACT_CLASSES, DOMAIN_BINS) or len_sum.shape != (B, TRACT_CLASSES):
        raise ValueError("hist is [B, 27, 128], len_sum [B, 27] of the tree's B branches")
    tracts = hist.sum(axis=2, dtype=np.uint64).astype(np.float64).reshape(B, 3, 3, 3)   # [b, direction, left, right]
    sites = len_sum.astype(np.float64).reshape(B, 3, 3, 3)
    ns = float(samples)
    groups = {name: [key] for name, key in TRACT_EVENTS.items()}
    groups["mixed"] = [(2, l, r) for l in (0, 1) for r in (0, 1)]
    groups["open"] = [(d, l, r) for d in range(3) for l in range(3) for r in range(3) if l == 2 or r == 2]
    out, total = {}, {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for name, keys in groups.items():
            count = sum(tracts[:, d, l, r] for d, l, r in keys)
            total[name] = sum(sites[:, d, l, r] for d, l, r in keys)
            out[name] = count / ns
            out[name + "_size"] = total[name] / count
        out["net_edge_sites"] = (total["grew_left"] + total["grew_right"] - total["shrank_left"] - total["shrank_right"]) / ns
    return out


def write_change_tracts(path, branch_names, samples, hist, len_sum):
    """the file of epievo_est_histories -X: the closed result, integers only; branch_names = the child node's name
    of every branch"""
    hist, len_sum = np.ascontiguousarray(hist, np.uint64), np.ascontiguousarray(len_sum, np.uint64)
    B = len(branch_names)
    if hist.shape != (B, TRACT_CLASSES, DOMAIN_BINS) or len_sum.shape != (B, TRACT_CLASSES):
        raise ValueError("hist is [branches, 27, 128], len_sum [branches, 27]")
    a, b = (hist, len_sum) if B else (np.zeros(1, np.uint64), np.zeros(1, np.uint64))
    if lib().epvh_write_change_tracts(path.encode(), "\n".join(branch_names).encode(), int(samples),
                                      _p(a, C.c_uint64), _p(b, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())


def read_change_tracts(path):
    """-> dict(samples, branch_names, hist uint64 [B, 27, 128], len_sum uint64 [B, 27])"""
    L = lib()
    h = L.epvh_read_change_tracts(path.encode())
    if not h:
        raise RuntimeError(L.epvh_last_error().decode())
    try:
        ns, B, ln = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.epvh_change_tracts_dims(h, C.byref(ns), C.byref(B), C.byref(ln))
        B = int(B.value)
        buf = C.create_string_buffer(int(ln.value))
        hist, len_sum = np.zeros((B, TRACT_CLASSES, DOMAIN_BINS), np.uint64), np.zeros((B, TRACT_CLASSES), np.uint64)
        a, b = (hist, len_sum) if B else (np.zeros(1, np.uint64), np.zeros(1, np.uint64))
        L.epvh_change_tracts_copy(h, buf, len(buf), _p(a, C.c_uint64), _p(b, C.c_uint64))
        return dict(samples=int(ns.value), branch_names=buf.value.decode().split("\n") if B else [], hist=hist,
                    len_sum=len_sum)
    finally:
        L.epvh_change_tracts_free(h)


# ---- spatial correlations (two-point counts of node states and branch changes along the genome)
def _corr_dims(n11, edges):
    bad = ValueError("a part is n11 [R, L + 1] with 1 <= L <= 1024 and edges [samples, R, 2, ceil(L / 64)]")
    if n11.ndim != 2 or edges.ndim != 4:
        raise bad
    R, L = n11.shape[0], n11.shape[1] - 1
    if L < 1 or L > 1024 or edges.shape[1:] != (R, 2, (L + 63) // 64):
        raise bad
    return R, L, edges.shape[0]


def corr_parts_merge(parts):
    """parts: [(sites, n11 [R, L + 1], edges [samples, R, 2, LW])] of adjacent stretches of sites in genome order, of
    the same samples, each of at least L sites -> the part of their union, (sites, n11, edges)"""
    if not parts:
        raise ValueError("no parts")
    cnts = np.array([int(p[0]) for p in parts], np.uint64)
    n11s = [np.ascontiguousarray(p[1], np.uint64) for p in parts]
    edges = [np.ascontiguousarray(p[2], np.uint64) for p in parts]
    R, L, ns = _corr_dims(n11s[0], edges[0])
    for a, e in zip(n11s, edges):
        if a.shape != n11s[0].shape or e.shape != edges[0].shape:
            raise ValueError("the parts differ in rows, max_lag or samples")
    n11, out = np.zeros((R, L + 1), np.uint64), np.zeros(edges[0].shape, np.uint64)
    o = out if out.size else np.zeros(1, np.uint64)
    total = C.c_uint64(0)
    if lib().epvh_corr_parts_merge(len(parts), R, L, ns, _p(cnts, C.c_uint64), _ptrs(n11s),
                                   _ptrs([e if e.size else np.zeros(1, np.uint64) for e in edges]),
                                   _p(n11 if n11.size else np.zeros(1, np.uint64), C.c_uint64), _p(o, C.c_uint64),
                                   C.byref(total)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return int(total.value), n11, out


def corr_part_close(sites, n11, edges):
    """a part over the whole genome of `sites` sites -> (n11, left1, right1), each [R, L + 1]: left1[r][d] (right1)
    are the ones at the left (right) site of the samples x (sites - d) pairs of lag d"""
    n11, edges = np.ascontiguousarray(n11, np.uint64), np.ascontiguousarray(edges, np.uint64)
    R, L, ns = _corr_dims(n11, edges)
    left1, right1 = np.zeros((R, L + 1), np.uint64), np.zeros((R, L + 1), np.uint64)
    one = np.zeros(1, np.uint64)
    if lib().epvh_corr_part_close(R, L, ns, int(sites), _p(n11 if R else one, C.c_uint64),
                                  _p(edges if edges.size else one, C.c_uint64), _p(left1 if R else one, C.c_uint64),
                                  _p(right1 if R else np.zeros(1, np.uint64), C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return n11.copy(), left1, right1


def spatial_correlation_summary(samples, n_sites, n11, left1, right1, tree):
    """a closed result -> dict: p11, p10, p01, p00 (float64 [R, L + 1], the joint frequencies of (X[p], X[p + d]) over
    the samples x (n_sites - d) pairs of lag d), corr (their Pearson correlation, nan where a margin is 0 or 1) and
    decay (per row the first lag >= 1 at which corr falls below 1/e, or None)"""
    n11, left1, right1 = (np.asarray(a, np.uint64).astype(np.float64) for a in (n11, left1, right1))
    R = 2 * tree.n_nodes - 1
    if n11.ndim != 2 or n11.shape[0] != R or left1.shape != n11.shape or right1.shape != n11.shape:
        raise ValueError("n11, left1 and right1 are [N + B, L + 1] of the tree's N nodes and B branches")
    L = n11.shape[1] - 1
    pairs = float(samples) * (float(n_sites) - np.arange(L + 1, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        p11, pl, pr = n11 / pairs, left1 / pairs, right1 / pairs
        var = pl * (1.0 - pl) * pr * (1.0 - pr)
        corr = np.where(var > 0.0, (p11 - pl * pr) / np.sqrt(var), np.nan)
    decay = []
    for r in range(R):
        below = np.nonzero(corr[r, 1:] < np.exp(-1.0))[0]
        decay.append(int(below[0]) + 1 if len(below) else None)
    return dict(p11=p11, p10=pl - p11, p01=pr - p11, p00=1.0 - pl - pr + p11, corr=corr, decay=decay)


def write_spatial_correlation(path, node_names, samples, n_sites, n11, left1, right1):
    """the file of epievo_est_histories -C: the closed result, integers only; node_names = the N node names"""
    n11, left1, right1 = (np.ascontiguousarray(a, np.uint64) for a in (n11, left1, right1))
    R = 2 * len(node_names) - 1
    if n11.ndim != 2 or n11.shape[0] != R or n11.shape[1] < 2 or left1.shape != n11.shape or right1.shape != n11.shape:
        raise ValueError("n11, left1 and right1 are [2 nodes - 1, L + 1]")
    if lib().epvh_write_spatial_correlation(path.encode(), "\n".join(node_names).encode(), int(samples), int(n_sites),
                                            n11.shape[1] - 1, _p(n11, C.c_uint64), _p(left1, C.c_uint64),
                                            _p(right1, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())


def read_spatial_correlation(path):
    """-> dict(samples, sites, max_lag, row_names ("NODE:<name>" / "BRANCH:<name>"), n11, left1, right1 uint64
    [R, L + 1])"""
    L_ = lib()
    h = L_.epvh_read_spatial_correlation(path.encode())
    if not h:
        raise RuntimeError(L_.epvh_last_error().decode())
    try:
        ns, n, ml, R, ln = (C.c_uint64(0) for _ in range(5))
        L_.epvh_spatial_correlation_dims(h, C.byref(ns), C.byref(n), C.byref(ml), C.byref(R), C.byref(ln))
        R, ml = int(R.value), int(ml.value)
        buf = C.create_string_buffer(int(ln.value))
        arrs = [np.zeros((R, ml + 1), np.uint64) for _ in range(3)]
        ptrs = [_p(a if a.size else np.zeros(1, np.uint64), C.c_uint64) for a in arrs]
        L_.epvh_spatial_correlation_copy(h, buf, len(buf), *ptrs)
        return dict(samples=int(ns.value), sites=int(n.value), max_lag=ml,
                    row_names=buf.value.decode().split("\n") if R else [], n11=arrs[0], left1=arrs[1], right1=arrs[2])
    finally:
        L_.epvh_spatial_correlation_free(h)


# ---- domain maps (per node, size and site: the samples in which the site lies in a run of at least that size)
DOMAIN_MAP_MAX_SIZE, DOMAIN_MAP_MAX_SIZES = 1024, 4


def domain_map_sizes(sizes):
    """-> uint32 [K]: 1 .. 4 strictly increasing sizes of 1 .. 1024, or ValueError"""
    z = [int(L) for L in np.atleast_1d(sizes)]
    if not 1 <= len(z) <= DOMAIN_MAP_MAX_SIZES:
        raise ValueError("domain maps take 1 .. %d sizes" % DOMAIN_MAP_MAX_SIZES)
    if any(L < 1 or L > DOMAIN_MAP_MAX_SIZE for L in z):
        raise ValueError("a size of the domain maps is 1 .. %d" % DOMAIN_MAP_MAX_SIZE)
    if any(b <= a for a, b in zip(z[:-1], z[1:])):
        raise ValueError("the sizes of the domain maps are strictly increasing")
    return np.array(z, np.uint32)


def domain_map_edge_bits(sizes):
    """E = 2 (L_K - 1): the bits of an edge record, and the fewest sites a part holds"""
    return 2 * (int(domain_map_sizes(sizes)[-1]) - 1)


def _pack_rows(x):
    """0/1 [R, n] -> uint64 [R, ceil(n / 64)], bit j of a row in word j // 64 at position j % 64"""
    x = np.ascontiguousarray(x, np.uint8)
    R, n = x.shape
    pad = np.zeros((R, (n + 63) // 64 * 64), np.uint8)
    pad[:, :n] = x != 0
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view("<u8").reshape(R, -1).astype(np.uint64)


def domain_map_members(x, L):
    """the opening of the 0/1 string x by L: uint8 [n], 1 where the site lies in a run of at least L ones"""
    x = np.asarray(x, np.uint8).reshape(1, -1)
    n = x.shape[1]
    w = _pack_rows(x)[0] if n else np.zeros(1, np.uint64)
    out = np.zeros(max((n + 63) // 64, 1), np.uint64)
    if lib().epvh_domain_map_members(_p(w, C.c_uint64), n, int(L), _p(out, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return np.unpackbits(out.astype("<u8").view(np.uint8), bitorder="little")[:n]


def domain_maps_part(x, sizes):
    """one sample over a stretch of sites: x 0/1 [N, cnt], 1 where the node is in the state asked for -> the part
    (cnt, counts uint32 [N, K, cnt], edges uint64 [1, N, 2, EW]) as the device counts it"""
    x = np.asarray(x, np.uint8)
    z = domain_map_sizes(sizes)
    N, cnt = x.shape
    EW = (domain_map_edge_bits(z) + 63) // 64
    counts, edges = np.zeros((N, len(z), cnt), np.uint32), np.zeros((1, N, 2, EW), np.uint64)
    one32, one64 = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    bits = _pack_rows(x)
    if lib().epvh_domain_maps_part(N, len(z), _p(z, C.c_uint32), cnt, _p(bits if bits.size else one64, C.c_uint64),
                                   _p(counts if counts.size else one32, C.c_uint32),
                                   _p(edges if edges.size else one64, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return cnt, counts, edges


def domain_maps_merge(sizes, parts):
    """parts: [(sites, counts [N, K, sites], edges [samples, N, 2, EW])] of adjacent stretches of sites in genome
    order, of the same samples, each of at least E = 2 (L_K - 1) sites -> the part of their union, (sites, counts,
    edges)"""
    if not parts:
        raise ValueError("no parts")
    z = domain_map_sizes(sizes)
    EW = (domain_map_edge_bits(z) + 63) // 64
    cnts = np.array([int(p[0]) for p in parts], np.uint64)
    counts = [np.ascontiguousarray(p[1], np.uint32) for p in parts]
    edges = [np.ascontiguousarray(p[2], np.uint64) for p in parts]
    N, ns = counts[0].shape[0], edges[0].shape[0]
    for n, a, e in zip(cnts, counts, edges):
        if a.shape != (N, len(z), int(n)) or e.shape != (ns, N, 2, EW):
            raise ValueError("a part is counts [N, K, sites] and edges [samples, N, 2, ceil((L_K - 1) / 32)] of the same "
                             "nodes, sizes and samples")
    out_c, out_e = np.zeros((N, len(z), int(cnts.sum())), np.uint32), np.zeros((ns, N, 2, EW), np.uint64)
    one32, one64 = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    cp = (C.POINTER(C.c_uint32) * len(parts))(*[_p(a if a.size else one32, C.c_uint32) for a in counts])
    total = C.c_uint64(0)
    if lib().epvh_domain_maps_merge(len(parts), N, len(z), _p(z, C.c_uint32), ns, _p(cnts, C.c_uint64), cp,
                                    _ptrs([e if e.size else one64 for e in edges]),
                                    _p(out_c if out_c.size else one32, C.c_uint32),
                                    _p(out_e if out_e.size else one64, C.c_uint64), C.byref(total)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return int(total.value), out_c, out_e


def domain_map_windows(maps, W):
    """maps [N, K, n] of integer counts -> uint64 [N, K, ceil(n / W)]: the sums over windows of W consecutive sites"""
    maps = np.asarray(maps)
    W = int(W)
    if W < 1:
        raise ValueError("a window holds at least one site")
    if maps.ndim != 3 or not np.issubdtype(maps.dtype, np.integer):
        raise ValueError("maps are integer counts [N, K, n]")
    n = maps.shape[2]
    if not n:
        return np.zeros(maps.shape[:2] + (0,), np.uint64)
    return np.add.reduceat(maps.astype(np.uint64), np.arange(0, n, W), axis=2)


def domain_calls(samples, maps, size_index, support=0.5, min_sites=1):
    """the located domains of every node: per node the list of (first site, last site, mean support) of the maximal
    intervals of at least min_sites sites whose cells maps[v, size_index, p] / samples all reach `support`.  maps
    are the integer counts [N, K, n] of `samples` samples"""
    maps = np.asarray(maps)
    if maps.ndim != 3 or not np.issubdtype(maps.dtype, np.integer):
        raise ValueError("maps are integer counts [N, K, n]")
    samples = int(samples)
    if samples < 1:
        raise ValueError("domain calls need at least one sample")
    if not 0.0 < float(support) <= 1.0:
        raise ValueError("the support is in (0, 1]")
    row = maps[:, int(size_index)].astype(np.int64)
    calls = []
    for v in range(row.shape[0]):
        ok = np.concatenate([[0], (row[v] >= float(support) * samples).astype(np.int8), [0]])
        d = np.diff(ok)
        out = []
        for a, b in zip(np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]):     # sites a .. b - 1
            if b - a >= int(min_sites):
                out.append((int(a), int(b) - 1, float(row[v, a:b].sum()) / (float(samples) * float(b - a))))
        calls.append(out)
    return calls


def write_domain_maps(path, node_names, samples, state, sizes, n_sites, W, sums):
    """the file of epievo_est_histories -D: window sums [N, K, ceil(n_sites / W)] of the maps, integers only"""
    z = domain_map_sizes(sizes)
    sums = np.ascontiguousarray(sums, np.uint64)
    if int(W) < 1:
        raise ValueError("a window holds at least one site")
    if sums.shape != (len(node_names), len(z), (int(n_sites) + int(W) - 1) // int(W)):
        raise ValueError("sums are [nodes, sizes, ceil(n_sites / W)]")
    if lib().epvh_write_domain_maps(path.encode(), "\n".join(node_names).encode(), int(samples), int(state), len(z),
                                    _p(z, C.c_uint32), int(n_sites), int(W),
                                    _p(sums if sums.size else np.zeros(1, np.uint64), C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())


def read_domain_maps(path):
    """-> dict(samples, sites, window, state, sizes uint32 [K], node_names, sums uint64 [N, K, windows])"""
    L_ = lib()
    h = L_.epvh_read_domain_maps(path.encode())
    if not h:
        raise RuntimeError(L_.epvh_last_error().decode())
    try:
        w = np.zeros(7, np.uint64)
        L_.epvh_domain_maps_dims(h, _p(w, C.c_uint64))
        ns, n, W, state, N, K, ln = (int(v) for v in w)
        buf = C.create_string_buffer(ln)
        z, sums = np.zeros(K, np.uint32), np.zeros((N, K, (n + W - 1) // W), np.uint64)
        L_.epvh_domain_maps_copy(h, buf, len(buf), _p(z, C.c_uint32),
                                 _p(sums if sums.size else np.zeros(1, np.uint64), C.c_uint64))
        return dict(samples=ns, sites=n, window=W, state=state, sizes=z,
                    node_names=buf.value.decode().split("\n") if N else [], sums=sums)
    finally:
        L_.epvh_domain_maps_free(h)


# ---- chain mixing diagnostics (does a site's history move, and how long does its jump count remember itself)
def _mixing_moments(samples, pairs, S1, S2, Ck):
    """-> (mean [n], var [n], cov [K + 1, n]) of a site's jump count x over the samples: the plain estimators, the
    mean and the variance over all samples, cov[k] = C_k / pairs[k] - mean^2 (cov[0] = var; nan where pairs[k] = 0)"""
    S1, S2, Ck = (np.asarray(a, np.uint64).astype(np.float64) for a in (S1, S2, Ck))
    pairs = np.asarray(pairs, np.uint64).astype(np.float64)
    if Ck.ndim != 2 or pairs.shape != (Ck.shape[0] + 1,) or S1.shape != Ck.shape[1:] or S2.shape != S1.shape:
        raise ValueError("pairs is [K + 1], S1 and S2 are [sites], C is [K, sites]")
    if samples < 1:
        raise ValueError("the mixing diagnostics hold no sample")
    mean = S1 / float(samples)
    var = S2 / float(samples) - mean * mean
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = np.concatenate([var[None], Ck / pairs[1:, None] - mean * mean])
    cov[1:][pairs[1:] == 0] = np.nan
    return mean, var, cov


def _geyer_tau(rho):
    """integrated autocorrelation time of rho [K + 1, ...] (rho[0] = 1) by Geyer's initial positive sequence:
    tau = -1 + 2 sum of G_m = rho[2 m] + rho[2 m + 1] over m = 0, 1, .. while G_m > 0 (G_0 always; a lag without
    its partner, K even, is left out).  -> (tau, censored): censored where every G_m up to K was positive, so
    that the sum was cut by max_lag and tau is a lower bound"""
    G = rho[0:rho.shape[0] // 2 * 2:2] + rho[1::2]
    with np.errstate(invalid="ignore"):
        alive = np.logical_and.accumulate(np.concatenate([np.ones((1,) + G.shape[1:], bool), G[1:] > 0.0]), axis=0)
    tau = -1.0 + 2.0 * np.where(alive, G, 0.0).sum(axis=0)
    return tau, alive[-1] & (G[-1] > 0.0)


def mixing_summary(samples, moved_pairs, pairs, moved, S1, S2, Ck):
    """the counts of DeviceSampler.mixing(counts=True) -> dict, per site: move_rate = moved / moved_pairs (nan
    without a linked pair), mean and var of the site's jump count x over the samples, rho [K + 1, sites] with
    rho[k] = (C_k / pairs[k] - mean^2) / var, tau (Geyer's initial positive sequence over rho[1 .. K]),
    tau_censored (the sequence was still positive at max_lag: tau is a lower bound) and ess = samples / tau clipped
    to [1, samples]; also samples, moved_pairs, pairs.  Where var == 0 (x never changed) rho, tau and ess are nan:
    the move rate is what speaks there.
    rho is the plain estimator: both members of a pair are centred at the mean of ALL samples and scaled by the
    variance of all samples, and the pairs that a run boundary cuts are missing from C_k but not from the mean.  Its
    bias is of the order 1 / (length of a run): for an independent chain of runs of length B, E rho[k] is about
    -1 / B, and rho[k] at k close to B rests on few pairs.  Read tau of short runs (B = 50) per window
    (mixing_window_summary), not per site."""
    moved = np.asarray(moved, np.uint32).astype(np.float64)
    mean, var, cov = _mixing_moments(samples, pairs, S1, S2, Ck)
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.where(var > 0.0, cov / var, np.nan)
        tau, censored = _geyer_tau(rho)
        tau = np.where(var > 0.0, tau, np.nan)
        ess = np.where(tau > 0.0, float(samples) / tau, float(samples))
        ess = np.where(var > 0.0, np.clip(ess, 1.0, float(samples)), np.nan)
        rate = moved / float(moved_pairs) if moved_pairs else np.full(moved.shape, np.nan)
    return dict(samples=int(samples), moved_pairs=int(moved_pairs), pairs=np.asarray(pairs, np.uint64),
                move_rate=rate, mean=mean, var=var, rho=rho, tau=tau, tau_censored=censored & (var > 0.0), ess=ess)


def mixing_window_summary(W, samples, moved_pairs, pairs, moved, S1, S2, Ck, first_site=0):
    """the same counts, pooled over windows of W consecutive global sites (the rows start at global site first_site;
    a window is [w W, (w + 1) W)) -> dict per window from window first_site // W on: sites, moved (uint64 sums),
    move_rate = moved / (moved_pairs x sites), rho [K + 1, windows] with rho[k] = sum_p cov_k(p) / sum_p var(p) over
    the window's sites (usable at 50 samples, where a single site's rho is not; nan where no site of the window
    varies), tau and tau_censored of it, and first_window"""
    W = int(W)
    if W < 1:
        raise ValueError("a window holds at least one site")
    moved = np.asarray(moved, np.uint32).astype(np.uint64)
    _, var, cov = _mixing_moments(samples, pairs, S1, S2, Ck)
    n = moved.shape[0]
    g = first_site + np.arange(n, dtype=np.int64)
    w0 = first_site // W
    cuts = np.nonzero(np.concatenate([[True], g[1:] // W != g[:-1] // W]))[0] if n else np.zeros(0, np.int64)
    nw = int(g[-1] // W - w0 + 1) if n else 0
    if len(cuts) != nw:
        raise AssertionError("windows of consecutive sites")
    sites = np.diff(np.concatenate([cuts, [n]])) if n else np.zeros(0, np.int64)
    msum = np.add.reduceat(moved, cuts) if n else moved
    vsum = np.add.reduceat(var, cuts) if n else var
    csum = np.add.reduceat(cov, cuts, axis=1) if n else cov
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = np.where(vsum > 0.0, csum / vsum, np.nan)
        tau, censored = _geyer_tau(rho)
        tau = np.where(vsum > 0.0, tau, np.nan)
        rate = msum / (float(moved_pairs) * sites) if moved_pairs else np.full(nw, np.nan)
    return dict(window=W, first_window=int(w0), sites=sites.astype(np.int64), moved=msum, move_rate=rate, rho=rho,
                tau=tau, tau_censored=censored & (vsum > 0.0))


def write_mixing(path, samples, moved_pairs, pairs, summary):
    """the file of mixing diagnostics per window: the header (samples, moved_pairs, max_lag, pairs[1 .. K], window,
    first_window), then a line per window: index, sites, moved (the integer window sum), move_rate, rho[1 .. K], tau.
    summary = what mixing_window_summary returned; floats are written so that they read back bit for bit"""
    rho = np.asarray(summary["rho"], np.float64)
    K = rho.shape[0] - 1
    pairs = np.asarray(pairs, np.uint64)
    if pairs.shape != (K + 1,):
        raise ValueError("pairs is [K + 1]")
    with open(path, "w") as f:
        f.write("#epievo-mixing 1\n")
        f.write("samples %d\nmoved_pairs %d\nmax_lag %d\n" % (samples, moved_pairs, K))
        f.write("pairs %s\n" % " ".join(str(int(p)) for p in pairs[1:]))
        f.write("window %d\nfirst_window %d\n" % (summary["window"], summary["first_window"]))
        f.write("#window sites moved move_rate %s tau\n" % " ".join("rho_%d" % k for k in range(1, K + 1)))
        for i in range(len(summary["sites"])):
            vals = [summary["move_rate"][i]] + list(rho[1:, i]) + [summary["tau"][i]]
            f.write("%d %d %d %s\n" % (summary["first_window"] + i, summary["sites"][i], int(summary["moved"][i]),
                                       " ".join(repr(float(v)) for v in vals)))


def read_mixing(path):
    """-> dict(samples, moved_pairs, max_lag, pairs uint64[K + 1], window, first_window, sites int64[windows], moved
    uint64[windows], move_rate, rho [K + 1, windows] (rho[0] = 1 where any rho of the window is a number), tau)"""
    with open(path) as f:
        lines = [ln.split() for ln in f.read().splitlines()]
    if not lines or lines[0][:1] != ["#epievo-mixing"]:
        raise RuntimeError("%s is not a file of mixing diagnostics" % path)
    head = {ln[0]: ln[1:] for ln in lines[1:7]}
    try:
        K = int(head["max_lag"][0])
        out = dict(samples=int(head["samples"][0]), moved_pairs=int(head["moved_pairs"][0]), max_lag=K,
                   pairs=np.array([0] + [int(v) for v in head["pairs"]], np.uint64), window=int(head["window"][0]),
                   first_window=int(head["first_window"][0]))
        rows = [ln for ln in lines[7:] if ln and not ln[0].startswith("#")]
        if len(out["pairs"]) != K + 1 or any(len(r) != K + 5 for r in rows):
            raise ValueError("a line of the wrong length")
        if [int(r[0]) for r in rows] != list(range(out["first_window"], out["first_window"] + len(rows))):
            raise ValueError("windows out of order")
        out["sites"] = np.array([int(r[1]) for r in rows], np.int64)
        out["moved"] = np.array([int(r[2]) for r in rows], np.uint64)
        fl = np.array([[float(v) for v in r[3:]] for r in rows], np.float64).reshape(len(rows), K + 2)
    except (KeyError, IndexError, ValueError) as e:
        raise RuntimeError("%s: malformed file of mixing diagnostics (%s)" % (path, e))
    out["move_rate"], out["tau"] = fl[:, 0].copy(), fl[:, K + 1].copy()
    first = np.where(np.isnan(fl[:, 1:K + 1]).all(axis=1), np.nan, 1.0)
    out["rho"] = np.concatenate([first[None], fl[:, 1:K + 1].T])
    return out


# ---- change patterns (what happened across the branches of the tree at one site)
CHANGE_PATTERN_CLASSES =("one_branch", "parallel_gain", "parallel_loss", "gain_and_loss", "reverted_only")


def change_pattern_row_names(tree):
    """the names of the R = 12 + 2 (N-1) + I rows, in order: the -P file's #rows line"""
    names = ["jumps_%d" % h for h in range(1, 7)] + ["jumps_7plus"] + list(CHANGE_PATTERN_CLASSES)
    nodes = range(1, tree.n_nodes)
    names += ["sole_gain:" + tree.node_names[v] for v in nodes] + ["sole_loss:" + tree.node_names[v] for v in nodes]
    return names + ["clade_changed:" + tree.node_names[v] for v in nodes if tree.subtree_sizes[v] > 1]


def change_pattern_summary(samples, rows, tree):
    """rows [R, ...] (per site, or window sums divided by the window's sites) -> dict of probabilities per sample:
    conserved (by descent: no jump on the tree), jump_spectrum [8, ...] (K = 0, 1 .. 6, >= 7), the five classes of
    CHANGE_PATTERN_CLASSES, sole_gain / sole_loss [N-1, ...] per branch, clade_nodes [I] and
    clade_identical_by_descent [I, ...] (no jump strictly below the internal non-root node)"""
    rows = np.asarray(rows)
    B = tree.n_nodes - 1
    clade_nodes = np.array([v for v in range(1, tree.n_nodes) if tree.subtree_sizes[v] > 1], np.uint32)
    if rows.shape[0] != 12 + 2 * B + len(clade_nodes):
        raise ValueError("rows holds %d rows, the tree has 12 + 2 x %d + %d" % (rows.shape[0], B, len(clade_nodes)))
    if samples < 1:
        raise ValueError("the change patterns hold no sample")
    p = rows.astype(np.float64) / float(samples)
    conserved = 1.0 - rows[:7].sum(axis=0, dtype=np.uint64).astype(np.float64) / float(samples)
    out = dict(conserved=conserved, jump_spectrum=np.concatenate([conserved[None], p[:7]]),
               sole_gain=p[12:12 + B], sole_loss=p[12 + B:12 + 2 * B], clade_nodes=clade_nodes,
               clade_identical_by_descent=1.0 - p[12 + 2 * B:])
    for i, name in enumerate(CHANGE_PATTERN_CLASSES):
        out[name] = p[7 + i]
    return out


# ---- epoch statistics (J and D per branch and epoch of the branch)
def epoch_edges(fixT, P):
    """E_p = floor(p fixT / P), p = 0 .. P-1 (uint64[P]): the epoch edges on a branch's fixed-point clock;
    the last epoch is open-ended"""
    out = np.zeros(int(P), np.uint64)
    lib().epvh_epoch_edges(int(fixT), int(P), _p(out, C.c_uint64))
    return out


def epoch_raw_add(parts):
    """raw parts uint64 [N-1, P, 32] (J[8], lo[8], hi[8], cov[8]) of the contexts of one genome -> their sum,
    with part = lo + 2^32 hi renormalised to lo < 2^32 so that no word wraps however many parts are added"""
    m = np.uint64(0xffffffff)
    tot = None
    for raw in parts:
        raw = np.array(raw, np.uint64)
        raw[..., 16:24] += raw[..., 8:16] >> np.uint64(32)
        raw[..., 8:16] &= m
        if tot is None:
            tot = raw
            continue
        if raw.shape != tot.shape:
            raise ValueError("raw parts of different shapes")
        tot = tot + raw          # (J and cov modulo 2^64: cov is two's complement)
        tot[..., 16:24] += tot[..., 8:16] >> np.uint64(32)
        tot[..., 8:16] &= m
    if tot is None:
        raise ValueError("no raw part")
    return tot


def epoch_close(raw, fixT):
    """raw uint64 [N-1, P, 32], fixT [N-1] -> (J int64 [N-1, P, 8], D [N-1, P, 8] Python ints in an object
    array): the closed counts, D[p] = part[p] + (E_p+1 - E_p) sum_{q <= p} cov[q]"""
    raw = np.ascontiguousarray(raw, np.uint64)
    f = np.ascontiguousarray(fixT, np.uint64)
    if raw.ndim != 3 or raw.shape[2] != 32 or f.shape != (raw.shape[0],):
        raise ValueError("raw is [N-1, P, 32], fixT [N-1]")
    closed = _epoch_closed_words(raw, f)
    D = closed[..., 8:16].astype(object) + closed[..., 16:24].astype(object) * (1 << 64)
    return closed[..., :8].astype(np.int64), D


def _epoch_closed_words(raw, f):
    closed = np.zeros(raw.shape[:2] + (24,), np.uint64)
    if raw.size and lib().epvh_epoch_close(_p(raw, C.c_uint64), _p(f, C.c_uint64), raw.shape[0], raw.shape[1],
                                           _p(closed, C.c_uint64)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return closed


def epoch_finish(raw, fixT, k, samples, counts=False):
    """what every sampler's epoch_stats() returns from a genome's raw part: (samples, J, D) per sample, or
    the closed integers with counts=True"""
    raw = np.ascontiguousarray(raw, np.uint64)
    f = np.ascontiguousarray(fixT, np.uint64)
    if counts:
        return (samples,) + epoch_close(raw, f)
    if not samples:
        raise RuntimeError("epoch statistics hold no sample")
    closed = _epoch_closed_words(raw, f)
    kk = np.ascontiguousarray(k, np.intc)
    J, D = np.zeros(raw.shape[:2] + (8,)), np.zeros(raw.shape[:2] + (8,))
    if raw.size and lib().epvh_epoch_counts_to_stats(_p(closed, C.c_uint64), _p(kk, C.c_int), raw.shape[0], raw.shape[1],
                                                     int(samples), _p(J, C.c_double), _p(D, C.c_double)):
        raise RuntimeError(lib().epvh_last_error().decode())
    return samples, J, D


def epoch_rate_factors(J, D, rates):
    """J, D [N-1, P, 8] -> rho[N-1, P] = sum_c J / sum_c D_c rate_c: per branch and epoch the multiplier of
    the fitted rates that maximises the likelihood of that epoch's counts (regional_rate_factor over the
    (branch, epoch) axes); NaN where an epoch has no dwell time"""
    J = np.ascontiguousarray(J, np.float64)
    D = np.ascontiguousarray(D, np.float64)
    if J.ndim != 3 or J.shape != D.shape or J.shape[2] != 8:
        raise ValueError("J and D are [N-1, P, 8], rates [8]")
    return regional_rate_factors(J.reshape(-1, 1, 8), D.reshape(-1, 1, 8), rates).reshape(J.shape[:2])


def _closed_words(J, D):
    J = np.asarray(J)
    closed = np.zeros(J.shape[:2] + (24,), np.uint64)
    closed[..., :8] = J.astype(np.int64).view(np.uint64)
    Do = np.asarray(D, object)
    closed[..., 8:16] = (Do % (1 << 64)).astype(np.uint64)
    closed[..., 16:24] = (Do // (1 << 64)).astype(np.uint64)
    return closed


def write_epoch_stats(path, node_names, branches, scale_exp, fixT, samples, J, D, rates):
    """the file of epievo_est_histories -E.  node_names, branches, scale_exp, fixT: per node, the root first;
    J int64 [N-1, P, 8] and D (Python ints) [N-1, P, 8]: the closed counts"""
    closed = _closed_words(J, D)
    br = np.ascontiguousarray(branches, np.float64)
    k = np.ascontiguousarray(scale_exp, np.intc)
    f = np.ascontiguousarray(fixT, np.uint64)
    r = np.ascontiguousarray(rates, np.float64)
    if lib().epvh_write_epoch_stats(path.encode(), "\n".join(node_names).encode(), len(br), closed.shape[1],
                                    _p(br, C.c_double), _p(k, C.c_int), _p(f, C.c_uint64), _p(closed, C.c_uint64),
                                    int(samples), _p(r, C.c_double)):
        raise RuntimeError(lib().epvh_last_error().decode())


def read_epoch_stats(path):
    """-> dict(samples, epochs, node_names, branches, scale_exp (non-root nodes), J int64 [N-1, P, 8], D Python
    ints [N-1, P, 8], start [N-1, P], factor [N-1, P])"""
    L = lib()
    h = L.epvh_read_epoch_stats(path.encode())
    if not h:
        raise RuntimeError(L.epvh_last_error().decode())
    try:
        ns, P, B, nl = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.epvh_epoch_stats_dims(h, C.byref(ns), C.byref(P), C.byref(B), C.byref(nl))
        P, B = int(P.value), int(B.value)
        buf = C.create_string_buffer(int(nl.value))
        br, k = np.zeros(max(B, 1)), np.zeros(max(B, 1), np.intc)
        closed = np.zeros((B, P, 24), np.uint64)
        st, f = np.zeros((B, P)), np.zeros((B, P))
        L.epvh_epoch_stats_copy(h, buf, len(buf), _p(br, C.c_double), _p(k, C.c_int), _p(closed, C.c_uint64),
                                _p(st, C.c_double), _p(f, C.c_double))
        D = closed[..., 8:16].astype(object) + closed[..., 16:24].astype(object) * (1 << 64)
        return dict(samples=int(ns.value), epochs=P, node_names=buf.value.decode().split("\n"), branches=br[:B],
                    scale_exp=k[:B], J=closed[..., :8].astype(np.int64), D=D, start=st, factor=f)
    finally:
        L.epvh_epoch_stats_free(h)
