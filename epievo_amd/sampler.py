"""ctypes binding of libepievo_mi355x.so (the C ABI of include/epievo_mi355x.h) and a
Python mirror of the reference's SingleSiteSampler interface on top of it
(/root/reference/src/libepievo/SingleSiteSampler.hpp:35-81: ctor(burn_in, batch),
reset(model, paths), run_mcmc(...) -> J, D, acc_rate).

There is no CPU fallback: if the HIP library is missing or no GPU can be opened,
construction raises."""
import ctypes as C
import functools
import os

import numpy as np

from . import _build
from . import host
from .host import FlatPaths
from .summaries import CHAIN, LIFECYCLE, _per_sample, _window_range, summary_method

_lib = None

EPV_OK, EPV_ERR_ARG, EPV_ERR_HIP, EPV_ERR_CAPACITY, EPV_ERR_STATE = 0, 1, 2, 3, 4


class EpvError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("epv error %d: %s" % (code, msg))
        self.code = code


class CapacityError(EpvError):
    pass


class _Counters(C.Structure):
    _fields_ = [("n_overflow", C.c_uint64), ("n_coop_tasks", C.c_uint64),
                ("n_sweeps", C.c_uint64), ("n_search_finished", C.c_uint64)]


MAX_CAPACITY = 2047    # EPV_MAX_CAP: jump slots per (site, branch)
EPOCH_MAX_P = 256      # EPV_EPOCH_MAX_P: epochs per branch of the epoch statistics
MIXING_MAX_LAG = 16    # EPV_MIX_MAX_LAG: lags of the mixing diagnostics


def _abi():
    """the C ABI of include/epievo_mi355x.h, declared once: name -> (argtypes, restype)"""
    i, u32, u64, vp = C.c_int, C.c_uint32, C.c_uint64, C.c_void_p
    ip, dp, fp, u8p, u32p, u64p, i64p = (C.POINTER(t) for t in (C.c_int, C.c_double, C.c_float, C.c_uint8, C.c_uint32,
                                                                C.c_uint64, C.c_int64))
    args = {   # every entry point returns an EPV_* code (int) but those of `other` below
        "epv_create": [i], "epv_destroy": [vp], "epv_last_error": [vp],
        "epv_set_tree": [vp, i, u32p, u32p, dp], "epv_set_model": [vp, dp, dp],
        "epv_upload_paths": [vp, u64, u8p, u64p, dp, u32, u64],
        "epv_set_capacity": [vp, u32], "epv_get_capacity": [vp, u32p],
        "epv_init_paths_indep": [vp, u64, u8p, u8p, u64, u32],
        "epv_indep_expectation": [vp, dp, dp, dp], "epv_indep_sufficient_statistics": [vp, dp, dp],
        "epv_indep_update_paths": [vp, dp, u64, u32], "epv_indep_node_posterior": [vp, dp, dp],
        "epv_set_global_length": [vp, u64], "epv_set_update_range": [vp, u64, u64], "epv_set_halo": [vp, u64, u64],
        "epv_halo_phases_left": [vp, u64p],
        "epv_reset": [vp], "epv_reset_async": [vp],
        "epv_sweep": [vp, u64, u64, u32, u64p], "epv_sweep_phase": [vp, i, u64, u32, u64p],
        "epv_run_mcmc": [vp, u64, u64, u64, u32, dp, dp, u64p],
        "epv_run_mcmc_sums": [vp, u64, u64, u64, u32, i, dp, dp, u64p],
        "epv_get_sufficient_statistics": [vp, dp, dp], "epv_scale_jump_times": [vp, dp],
        "epv_paths_total_jumps": [vp, u64p], "epv_download_paths": [vp, u8p, u64p, dp], "epv_get_tri_llh": [vp, dp],
        "epv_column_bytes": [vp],
        "epv_get_columns": [vp, u64, u64, vp], "epv_put_columns": [vp, u64, u64, vp],
        "epv_copy_columns": [vp, u64, u64, vp, u64], "epv_copy_columns_async": [vp, u64, u64, vp, u64, i],
        "epv_dev_alloc": [vp, u64, C.POINTER(vp)], "epv_dev_free": [vp, vp],
        "epv_run_mcmc_counts": [vp, u64, u64, u64, u32, i64p, u64p], "epv_counts_to_stats": [vp, i64p, u64, i, dp, dp],
        "epv_get_counters": [vp, C.POINTER(_Counters)], "epv_kernel_time_ms": [vp, dp, u64p], "epv_set_timing": [vp, i],
        "epv_pack_columns_dev": [vp, u64, u64, vp], "epv_unpack_columns_dev": [vp, u64, u64, vp],
        "epv_device_of": [vp], "epv_dev_write": [vp, vp, vp, u64], "epv_dev_read": [vp, vp, vp, u64],
        "epv_set_options": [vp, u32], "epv_get_options": [vp, u32p],
        "epv_phase_mode": [vp, u32p], "epv_phase_plan": [vp, u32p],
        "epv_philox_kat": [vp, u64, u32, u32p, dp], "epv_math_kat": [vp, u32, u32, u32, dp, dp],
        "epv_merge_kat": [vp, u32, u32p, dp, dp, u32p],
        "epv_trial_kat": [vp, u64, u32, u32p, dp, u32p, dp],
        "epv_direct_kat": [vp, u64, u32, u32p, dp, u32p, dp], "epv_direct_giveups": [vp, u64p],
        "epv_set_unobserved": [vp, u8p], "epv_unobserved_cells": [vp, u64p],
        "epv_set_leaf_evidence": [vp, fp], "epv_leaf_evidence_cells": [vp, u64p],
        "epv_set_fixed_sites": [vp, u8p], "epv_fixed_sites": [vp, u64p],
        "epv_forward_simulate": [vp, u64, u8p, u64, u32, u64p], "epv_forward_last_ms": [vp, dp, dp],
        # the summaries: what is particular to each (the four lifecycle entry points of each follow from CHAIN)
        "epv_get_path_average": [vp, u64, u64, u32p], "epv_path_average_layout": [vp, u32p, u64p, u64p],
        "epv_branch_events_set_samples": [vp, u64], "epv_branch_events_layout": [vp, u64p, u64p],
        "epv_get_branch_events": [vp, u64, u64, u32p], "epv_get_branch_event_windows": [vp, u64, u64, u64, u64p],
        "epv_window_stats_set_samples": [vp, u64], "epv_window_stats_scale_exps": [vp, ip],
        "epv_window_stats_layout": [vp, u64p, u64p, u64p], "epv_get_window_stats": [vp, u64, u64, i64p],
        "epv_window_counts_to_stats": [vp, i64p, u64, u64, dp, dp],
        "epv_epoch_stats_set_samples": [vp, u64], "epv_epoch_stats_layout": [vp, u32p, u32p, ip, u64p],
        "epv_get_epoch_stats": [vp, u64p],
        "epv_lineage_origins_set_samples": [vp, u64], "epv_lineage_origins_layout": [vp, u32p, u32p, u64p, u64p],
        "epv_lineage_origin_rows": [vp, u32p, u32p], "epv_lineage_origins_scale_exp": [vp, ip],
        "epv_get_lineage_origins": [vp, u64, u64, u32p, u64p],
        "epv_get_lineage_origin_windows": [vp, u64, u64, u64, u64p],
        "epv_domain_stats_layout": [vp, u32p, u32p, u64p, u64p, u64p], "epv_get_domain_stats": [vp, u64p, u64p, u64p],
        "epv_change_patterns_layout": [vp, u32p, u32p, u32p, u64p, u64p], "epv_get_change_patterns": [vp, u64, u64, u32p],
        "epv_get_change_pattern_windows": [vp, u64, u64, u64, u64p],
        "epv_domain_turnover_layout": [vp, u32p, u32p, u64p, u64p, u64p],
        "epv_get_domain_turnover": [vp, u64p, u64p, u64p],
        "epv_spatial_correlation_layout": [vp, u32p, u32p, u64p, u64p, u64p],
        "epv_get_spatial_correlation": [vp, u64p, u64p],
        "epv_mixing_layout": [vp, u64p, u64p, u32p], "epv_mixing_pairs": [vp, u64p],
        "epv_mixing_counts": [vp, u64, u64, u32p, u64p], "epv_mixing_windows": [vp, u64, u64, u64, u64p],
        "epv_domain_maps_layout": [vp, u32p, u32p, u32p, u32p, u64p, u64p, u64p], "epv_get_domain_maps": [vp, u32p, u64p],
        "epv_change_tracts_layout": [vp, u32p, u32p, u32p, u64p, u64p, u64p], "epv_get_change_tracts": [vp, u64p, u64p, u64p],
    }
    # epv_set_<stem>: what switches the summary on, after the context
    set_args = {"path_average": [u32], "branch_events": [i], "window_stats": [u64], "epoch_stats": [u32],
                "lineage_origins": [i], "domain_stats": [u64], "change_patterns": [i], "domain_turnover": [u64],
                "spatial_correlation": [u32, u64], "mixing": [u32], "domain_maps": [u32, u32p, u32, u64], "change_tracts": [u64]}
    for s in CHAIN:
        args["epv_set_" + s.stem] = [vp] + set_args[s.stem]
        args["epv_reset_" + s.stem] = args["epv_accumulate_" + s.stem] = [vp]
        args["epv_%s_samples" % s.stem] = [vp, u64p]
    other = {"epv_create": vp, "epv_destroy": None, "epv_last_error": C.c_char_p, "epv_column_bytes": u64}
    return {name: (a, other.get(name, i)) for name, a in args.items()}


ABI = _abi()
ABI_SYMBOLS = list(ABI)

# planes of the posterior branch-event maps (include/epievo_mi355x.h), in order
BRANCH_EVENT_PLANES = ("end1", "net_gain", "net_loss", "changed", "gains", "losses")
# the first rows of the change patterns (include/epievo_mi355x.h), in order; then sole_gain[b], sole_loss[b]
# per branch and clade_changed[j] per internal non-root node
CHANGE_PATTERN_ROWS = ("jumps_1", "jumps_2", "jumps_3", "jumps_4", "jumps_5", "jumps_6", "jumps_7plus", "one_branch",
                       "parallel_gain", "parallel_loss", "gain_and_loss", "reverted_only")


def lib():
    """Load the HIP library; raise (never fall back) when it has not been built."""
    global _lib
    if _lib is None:
        # EPIEVO_MI355X_LIB: another build of the same library (A/B runs of kernel variants)
        path = os.environ.get("EPIEVO_MI355X_LIB", _build.HIP_SO)
        if not os.path.exists(path):
            raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; "
                               "g.build()'` (hipcc --offload-arch=gfx950)" % path)
        L = C.CDLL(path)
        for name, (argtypes, restype) in ABI.items():
            fn = getattr(L, name)
            fn.argtypes, fn.restype = argtypes, restype
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class DevBuf:
    """Zero-filled device memory on a context's GPU.  torch (and anything else that speaks the
    CUDA array interface) sees it without a copy, so the halo columns a sharded run hands to
    RCCL never pass through the host."""

    def __init__(self, dev, nbytes):
        self.dev, self.nbytes = dev, int(nbytes)
        self.p = dev.dev_alloc(self.nbytes)
        self.ptr = int(self.p.value)

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2,
                "strides": None}

    def free(self):
        if self.p is not None and self.dev.h:
            self.dev.dev_free(self.p)
        self.p, self.ptr = None, 0


class DeviceSampler:
    """One context = one GPU.  Thin, explicit face of the C ABI."""

    def __init__(self, device=0):
        self.L = lib()
        self.h = self.L.epv_create(device)
        if not self.h:
            raise RuntimeError("epv_create(%d) failed: no usable HIP device (this build has no "
                               "CPU fallback)" % device)
        self.n_sites = self.n_nodes = self.B = 0
        self.n_global = 0             # genome length as upload_paths set it
        self.auto_grow = False     # True: widen the jump slots after an overflow and carry on
        self.capacity_events = []  # messages of the overflows that were absorbed
        self.halo = (0, 0)

    def close(self):
        if getattr(self, "h", None):
            self.L.epv_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def _ck(self, rc):
        if rc != EPV_OK:
            msg = self.L.epv_last_error(self.h).decode()
            raise (CapacityError if rc == EPV_ERR_CAPACITY else EpvError)(rc, msg)

    def _ck_mcmc(self, rc):
        """after an MCMC call: a capacity overflow leaves a valid chain (the over-long proposals
        were rejected) and complete outputs, so with auto_grow the slots are doubled for the
        following calls -- what the reference's std::vector paths do on their own -- and the
        call succeeds; otherwise it raises CapacityError like any other failure."""
        if rc == EPV_ERR_CAPACITY and self.auto_grow:
            msg = self.L.epv_last_error(self.h).decode()
            cap = self.capacity()
            if cap < MAX_CAPACITY:
                self.set_capacity(min(MAX_CAPACITY, 2 * cap))
                self.capacity_events.append(msg)
                return
        self._ck(rc)

    def _u64(self, fn):
        """an entry point whose one result is a uint64 out-parameter"""
        v = C.c_uint64(0)
        self._ck(fn(self.h, C.byref(v)))
        return int(v.value)

    def _window_range(self, W, first_window, n_windows):
        """(W, number of windows) of a read-out per window: all windows of the genome unless a range is given"""
        return _window_range(W, max(self.n_global, self.n_sites), first_window, n_windows)

    # what every summary has besides enable_<stem>, its layout and its read-outs: reset_<stem>, accumulate_<stem>
    # and <stem>_samples are made of these three, one set per row of SUMMARIES and DIAGNOSTICS (below the class)
    def _reset_summary(self, s):
        self._ck(getattr(self.L, "epv_reset_" + s.stem)(self.h))

    def _accumulate_summary(self, s):
        self._ck(getattr(self.L, "epv_accumulate_" + s.stem)(self.h))

    def _summary_samples(self, s):
        return self._u64(getattr(self.L, "epv_%s_samples" % s.stem))

    def set_options(self, reference_proposal_ratio=False, forward_rejection=False, sample_root=False):
        """see EPV_OPT_* in include/epievo_mi355x.h.  These three bits; EPV_OPT_DIRECT_SAMPLER and EPV_OPT_DIRECT_FUSED
        stay as set_direct_sampler left them and EPV_OPT_LEAF_FAST as set_leaf_fast did, so the order of the calls does
        not matter (forward_rejection while the direct sampler is on: EpvError)"""
        flags = C.c_uint32(0)
        self._ck(self.L.epv_get_options(self.h, C.byref(flags)))
        self._ck(self.L.epv_set_options(self.h, (1 if reference_proposal_ratio else 0) | (2 if forward_rejection else 0) |
                                        (4 if sample_root else 0) | (flags.value & (24 | 32))))

    def options(self):
        """the option word (EPV_OPT_* bits) as set_options and set_direct_sampler left it (epv_get_options)"""
        flags = C.c_uint32(0)
        self._ck(self.L.epv_get_options(self.h, C.byref(flags)))
        return int(flags.value)

    def set_direct_sampler(self, on=True, fused=False):
        """EPV_OPT_DIRECT_SAMPLER: jump times by the direct end-conditioned sampler, bounded work per segment (DESIGN
        7.22).  Its own call because set_options keeps its three keywords: it changes its bits of the word and leaves
        the others, as set_options leaves these.  With forward_rejection: EpvError.
        fused=True adds EPV_OPT_DIRECT_FUSED: where the default mode would run the fused phase, the direct mode runs
        the fused kernel's direct bodies (same results bit for bit, one launch per colour phase).  on=False clears both."""
        flags = C.c_uint32(0)
        self._ck(self.L.epv_get_options(self.h, C.byref(flags)))
        self._ck(self.L.epv_set_options(self.h, (flags.value & ~24) | ((8 | (16 if fused else 0)) if on else 0)))

    def set_leaf_fast(self, on=True):
        """EPV_OPT_LEAF_FAST: a held leaf cell (set_unobserved, set_leaf_evidence) keeps the fused phase, the second or
        the third proposal kernel, in their leaf variants, instead of sending every colour phase to the first kernel
        (DESIGN 7.23).  Same chain bit for bit; off by default.  Its own call, as set_direct_sampler is: it changes
        this bit of the word and leaves the others, and set_options / set_direct_sampler leave this one."""
        flags = C.c_uint32(0)
        self._ck(self.L.epv_get_options(self.h, C.byref(flags)))
        self._ck(self.L.epv_set_options(self.h, (flags.value & ~32) | (32 if on else 0)))

    def direct_giveups(self):
        """segments the direct sampler gave up on since the context was created (epv_direct_giveups)"""
        return self._u64(self.L.epv_direct_giveups)

    def direct_kat(self, seed, items, reals):
        """the direct end-conditioned sampler on known segments (epv_direct_kat): items[i] = (site, sweep, node,
        segment, room, start state | end state << 1, first draw index, 0), reals[i] = (T, r0, r1, start time).  Returns
        (uint32 [i, 4] = outcome, jumps, uniforms consumed, longest run of rounds; float64 [i, 8] = the first times)."""
        it = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1, 8)
        re = np.ascontiguousarray(reals, dtype=np.float64).reshape(-1, 4)
        if len(it) != len(re):
            raise ValueError("direct_kat: items and reals differ in length")
        w, d = np.zeros((len(it), 4), np.uint32), np.zeros((len(it), 8))
        self._ck(self.L.epv_direct_kat(self.h, int(seed), len(it), _p(it, C.c_uint32), _p(re, C.c_double),
                                       _p(w, C.c_uint32), _p(d, C.c_double)))
        return w, d

    PHASE_KERNELS = {
        0: "epv_mh_propose_kernel + epv_mh_jumps_kernel + epv_mh_accept_kernel",
        1: "epv_mh_propose2_kernel + epv_mh_jumps_all_kernel + epv_mh_accept_kernel",
        2: "epv_mh_propose2_kernel + epv_seg_search_kernel + epv_seg_assemble_kernel + epv_mh_accept_kernel",
        3: "epv_mh_propose2_kernel<fused>: proposal, segment search, assembly and acceptance in one launch",
        4: "epv_mh_propose3_kernel + epv_mh_jumps_all_kernel + epv_mh_accept3_kernel",
    }

    def phase_mode(self):
        """EPV_PHASE_* of include/epievo_mi355x.h: which kernels a colour phase launches.  (With the direct sampler
        on, the jump stage of the named family runs its direct variants; phase_plan()["direct"] says so.)"""
        v = C.c_uint32(0)
        self._ck(self.L.epv_phase_mode(self.h, C.byref(v)))
        return int(v.value)

    def phase_plan(self):
        """the kernel variants of a colour phase (epv_phase_plan, EPV_PLAN_* of include/epievo_mi355x.h); without a
        GPU: host.phase_plan"""
        v = C.c_uint32(0)
        self._ck(self.L.epv_phase_plan(self.h, C.byref(v)))
        return host.plan_fields(int(v.value))

    def philox_kat(self, seed, counters):
        """the device's Philox blocks (epv_philox_kat): counters[i] = (site, sweep, branch, segment, trial,
        block); returns [i, form, 2] doubles, form = inline-asm, plain, plain at a constant-folded call site"""
        ctr = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1, 6)
        out = np.zeros((ctr.shape[0], 3, 2))
        self._ck(self.L.epv_philox_kat(self.h, int(seed), ctr.shape[0], _p(ctr, C.c_uint32), _p(out, C.c_double)))
        return out

    def math_kat(self, op, items, where=0):
        """the arithmetic under the kernels on known inputs (epv_math_kat): items[i] = up to four doubles, the
        inputs of `op`; where = 0 a kernel of its own, 1 the library's host pass of the same headers.
        Returns [i, 6] doubles (an op's outputs first, zeros after)."""
        x = np.ascontiguousarray(items, dtype=np.float64)
        x = x.reshape(-1, 1) if x.ndim == 1 else x
        inp = np.zeros((x.shape[0], 4))
        inp[:, :x.shape[1]] = x
        out = np.zeros((x.shape[0], 6))
        self._ck(self.L.epv_math_kat(self.h, int(op), int(where), x.shape[0], _p(inp, C.c_double), _p(out, C.c_double)))
        return out

    def merge_kat(self, items):
        """the three-way merge of a triple's jumps on known inputs (epv_merge_kat): items[i] = (start states
        (l, m, r), (left times, middle times, right times) with 0 .. 8 each, branch length).  Returns
        (D [i, form, 8] doubles, J [i, form, 8] uint32), form 0 = merge3 with register accumulators,
        1 = merge3_sel with LDS accumulators behind the batched first-jump load."""
        n = len(items)
        heads = np.zeros(n, np.uint32)
        times = np.zeros((n, 25))
        for i, (init, cols, blen) in enumerate(items):
            h = 0
            for c in range(3):
                k = len(cols[c])
                if k > 8:
                    raise ValueError("merge_kat: at most 8 jumps per column")
                h |= (int(init[c]) & 1) << c | k << (4 + 4 * c)
                times[i, 8 * c:8 * c + k] = cols[c]
            heads[i] = h
            times[i, 24] = blen
        D = np.zeros((n, 2, 8))
        J = np.zeros((n, 2, 8), np.uint32)
        self._ck(self.L.epv_merge_kat(self.h, n, _p(heads, C.c_uint32), _p(times, C.c_double), _p(D, C.c_double),
                                      _p(J, C.c_uint32)))
        return D, J

    def trial_kat(self, seed, items, reals):
        """the trial evaluator of the end-conditioned sampler on known inputs (epv_trial_kat): items[i] = (site,
        sweep, node, segment, first trial, room, start | end << 1 | nielsen << 2, 0), reals[i] = (length, rate 0,
        rate 1, trunc, u0, start time).  Returns (W [i, 5, 4] uint32 = outcome, winning trial, jumps, M of the
        single-trial scan, run_trial on u0, and scan_trials over 1, 4, 8 trials; first [i] = the first draw;
        T [i, 5, 2] = the first two jump times)."""
        it = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1, 8)
        re = np.ascontiguousarray(reals, dtype=np.float64).reshape(-1, 6)
        n = it.shape[0]
        if re.shape[0] != n:
            raise ValueError("trial_kat: %d items, %d rows of reals" % (n, re.shape[0]))
        W = np.zeros((n, 5, 4), np.uint32)
        D = np.zeros((n, 11))
        self._ck(self.L.epv_trial_kat(self.h, int(seed), n, _p(it, C.c_uint32), _p(re, C.c_double), _p(W, C.c_uint32),
                                      _p(D, C.c_double)))
        return W, D[:, 0].copy(), D[:, 1:].reshape(n, 5, 2).copy()

    def set_unobserved(self, mask):
        """missing leaf data (epv_set_unobserved): mask[b-1, s] != 0 -> the leaf end state of branch b at
        local site s is resampled with the history instead of pinned.  Shape (n_nodes - 1, n_sites) or
        flat in that order, halo columns included; None clears.  Nonzero entries are allowed on leaf
        branches only.  Uploading paths clears the mask."""
        if mask is None:
            self._ck(self.L.epv_set_unobserved(self.h, None))
            return
        m = np.ascontiguousarray(mask).reshape(-1)
        if m.size != self.B * self.n_sites:
            raise ValueError("mask of unobserved cells: %d entries for %d branches x %d sites"
                             % (m.size, self.B, self.n_sites))
        m = (m != 0).astype(np.uint8)
        self._ck(self.L.epv_set_unobserved(self.h, _p(m, C.c_uint8)))

    def unobserved_cells(self):
        """the number of leaf cells flagged unobserved (epv_unobserved_cells)"""
        return self._u64(self.L.epv_unobserved_cells)

    def set_leaf_evidence(self, p_state1):
        """leaf evidence (epv_set_leaf_evidence): p_state1[b-1, s] = P(the leaf end state of branch b at local
        site s is 1 | that cell's own observation), float32, NaN = none.  Such a cell is resampled with the
        history from the leaf vector (1 - r, r); r = 0 or 1 is data, r = 0.5 an unobserved cell.  Shape
        (n_nodes - 1, n_sites) or flat in that order, halo columns included; None clears.  Non-NaN entries
        are allowed on leaf branches only; they win over the mask.  Uploading paths clears the table."""
        if p_state1 is None:
            self._ck(self.L.epv_set_leaf_evidence(self.h, None))
            return
        r = np.ascontiguousarray(p_state1, np.float32).reshape(-1)
        if r.size != self.B * self.n_sites:
            raise ValueError("table of leaf evidence: %d entries for %d branches x %d sites"
                             % (r.size, self.B, self.n_sites))
        self._ck(self.L.epv_set_leaf_evidence(self.h, _p(r, C.c_float)))

    def leaf_evidence_cells(self):
        """the number of leaf cells that hold evidence (epv_leaf_evidence_cells)"""
        return self._u64(self.L.epv_leaf_evidence_cells)

    def set_fixed_sites(self, mask):
        """fixed sites (epv_set_fixed_sites): mask[s] != 0 -> local site s is never changed by a colour phase, stays
        context for its neighbours, centres no counted triple and is not counted in n_accepted.  One entry per local
        column, halo columns included; None clears.  Regions are made of these (host.region_fixed_mask).  Uploading
        paths clears the mask; the seven summaries that count across neighbouring sites and the mask refuse each other."""
        if mask is None:
            self._ck(self.L.epv_set_fixed_sites(self.h, None))
            return
        m = np.ascontiguousarray(mask).reshape(-1)
        if m.size != self.n_sites:
            raise ValueError("mask of fixed sites: %d entries for %d sites" % (m.size, self.n_sites))
        m = (m != 0).astype(np.uint8)
        self._ck(self.L.epv_set_fixed_sites(self.h, _p(m, C.c_uint8)))

    def fixed_sites(self):
        """the number of fixed sites among those whose acceptances are counted (epv_fixed_sites)"""
        return self._u64(self.L.epv_fixed_sites)

    def capacity(self):
        v = C.c_uint32(0)
        self._ck(self.L.epv_get_capacity(self.h, C.byref(v)))
        return int(v.value)

    def set_capacity(self, capacity):
        self._ck(self.L.epv_set_capacity(self.h, int(capacity)))

    def set_tree(self, tree):
        self.n_nodes, self.B = tree.n_nodes, tree.n_nodes - 1
        self._ck(self.L.epv_set_tree(self.h, tree.n_nodes, _p(tree.parent_ids, C.c_uint32),
                                     _p(tree.subtree_sizes, C.c_uint32),
                                     _p(tree.branches, C.c_double)))

    def set_model(self, model):
        self._ck(self.L.epv_set_model(self.h, _p(model.rates, C.c_double), _p(model.T, C.c_double)))

    def upload_paths(self, fp, capacity=0, global_site_offset=0, n_global=None):
        jumps = fp.jumps if len(fp.jumps) else np.zeros(1)
        self.n_sites = fp.n_sites
        self._ck(self.L.epv_upload_paths(self.h, fp.n_sites, _p(fp.init, C.c_uint8),
                                         _p(fp.offsets, C.c_uint64), _p(jumps, C.c_double),
                                         capacity, global_site_offset))
        if n_global is not None:
            self._ck(self.L.epv_set_global_length(self.h, n_global))
        self.n_global = int(global_site_offset + fp.n_sites if n_global is None else n_global)
        self.halo = (0, 0)

    def init_paths_indep(self, root, leaf, seed, capacity=0):
        root = np.ascontiguousarray(root, np.uint8)
        leaf = np.ascontiguousarray(leaf, np.uint8)
        self.n_sites = len(root)
        self._ck(self.L.epv_init_paths_indep(self.h, len(root), _p(root, C.c_uint8),
                                             _p(leaf, C.c_uint8), seed, capacity))

    def forward_simulate(self, n_sites, seed, root=None, capacity=0):
        """epievo_sim's forward simulation on the device (set_tree and set_model first); the histories
        are resident afterwards.  Doubles the jump slots until every path fits -> total jumps"""
        self.n_sites = int(n_sites)
        rp = None
        if root is not None:
            root = np.ascontiguousarray(root, np.uint8)
            rp = _p(root, C.c_uint8)
        tot = C.c_uint64(0)
        cap = capacity or 16
        while True:
            rc = self.L.epv_forward_simulate(self.h, self.n_sites, rp, int(seed), cap, C.byref(tot))
            if rc == EPV_ERR_CAPACITY and cap < 2047:
                cap = min(2047, cap * 2)
                continue
            self._ck(rc)
            return int(tot.value)

    def forward_last_ms(self):
        """(device memory management, simulation) wall clock of the last forward_simulate, ms"""
        a, b = C.c_double(0), C.c_double(0)
        self._ck(self.L.epv_forward_last_ms(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def indep_expectation(self, rates):
        r = np.ascontiguousarray(rates, np.float64)
        J, D = np.zeros(self.B * 2), np.zeros(self.B * 2)
        self._ck(self.L.epv_indep_expectation(self.h, _p(r, C.c_double), _p(J, C.c_double), _p(D, C.c_double)))
        return J, D

    def indep_suffstats(self):
        J, D = np.zeros(self.B * 2), np.zeros(self.B * 2)
        self._ck(self.L.epv_indep_sufficient_statistics(self.h, _p(J, C.c_double), _p(D, C.c_double)))
        return J, D

    def indep_update_paths(self, rates, seed, sweep=0):
        r = np.ascontiguousarray(rates, np.float64)
        self._ck_mcmc(self.L.epv_indep_update_paths(self.h, _p(r, C.c_double), seed, sweep))

    def indep_node_posterior(self, rates):
        """-> (n_nodes, n_sites): P(state 1) at every node and site given all leaf data, the mask of
        unobserved cells and the table of leaf evidence, under the site-independent two-rate model
        (epv_indep_node_posterior): the imputed probability of every missing or soft leaf cell and the
        marginal ancestral reconstruction"""
        r = np.ascontiguousarray(rates, np.float64)
        out = np.zeros((self.n_nodes, self.n_sites))
        self._ck(self.L.epv_indep_node_posterior(self.h, _p(r, C.c_double), _p(out, C.c_double)))
        return out

    def set_update_range(self, first, last):
        self._ck(self.L.epv_set_update_range(self.h, first, last))

    def set_halo(self, left, right):
        self._ck(self.L.epv_set_halo(self.h, left, right))
        self.halo = (int(left), int(right))

    def halo_phases_left(self):
        return self._u64(self.L.epv_halo_phases_left)

    def reset(self):
        self._ck(self.L.epv_reset(self.h))

    def sweep(self, n_sweeps, seed, sweep_base=0):
        nacc = C.c_uint64(0)
        self._ck_mcmc(self.L.epv_sweep(self.h, n_sweeps, seed, sweep_base, C.byref(nacc)))
        return int(nacc.value)

    def sweep_phase(self, colour, seed, sweep):
        nacc = C.c_uint64(0)
        self._ck(self.L.epv_sweep_phase(self.h, colour, seed, sweep, C.byref(nacc)))
        return int(nacc.value)

    def run_mcmc(self, burn_in, batch, seed, sweep_base=0, average=True):
        J, D = np.zeros(self.B * 8), np.zeros(self.B * 8)
        nacc = C.c_uint64(0)
        self._ck_mcmc(self.L.epv_run_mcmc_sums(self.h, burn_in, batch, seed, sweep_base, int(average),
                                               _p(J, C.c_double), _p(D, C.c_double), C.byref(nacc)))
        return J, D, int(nacc.value)

    def suffstats(self):
        J, D = np.zeros(self.B * 8), np.zeros(self.B * 8)
        self._ck(self.L.epv_get_sufficient_statistics(self.h, _p(J, C.c_double), _p(D, C.c_double)))
        return J, D

    def scale_jump_times(self, new_branches):
        nb = np.ascontiguousarray(new_branches, dtype=np.float64)
        self._ck(self.L.epv_scale_jump_times(self.h, _p(nb, C.c_double)))

    def paths(self):
        tot = C.c_uint64(0)
        self._ck(self.L.epv_paths_total_jumps(self.h, C.byref(tot)))
        init = np.zeros(self.B * self.n_sites, np.uint8)
        off = np.zeros(self.B * self.n_sites + 1, np.uint64)
        jumps = np.zeros(max(tot.value, 1))
        self._ck(self.L.epv_download_paths(self.h, _p(init, C.c_uint8), _p(off, C.c_uint64),
                                           _p(jumps, C.c_double)))
        return FlatPaths(self.n_sites, self.n_nodes, init, off, jumps[:tot.value])

    def tri_llh(self):
        out = np.zeros(self.n_sites)
        self._ck(self.L.epv_get_tri_llh(self.h, _p(out, C.c_double)))
        return out

    def column_bytes(self):
        return int(self.L.epv_column_bytes(self.h))

    def get_columns(self, first, count):
        buf = np.zeros(count * self.column_bytes(), np.uint8)
        self._ck(self.L.epv_get_columns(self.h, first, count, buf.ctypes.data_as(C.c_void_p)))
        return buf

    def put_columns(self, first, count, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        self._ck(self.L.epv_put_columns(self.h, first, count, buf.ctypes.data_as(C.c_void_p)))

    # ---- several shards on one GPU (see epievo_amd.parallel.LocalGroup)
    def copy_columns_to(self, first, count, other, other_first):
        self._ck(self.L.epv_copy_columns(self.h, first, count, other.h, other_first))

    def dev_alloc(self, nbytes):
        p = C.c_void_p(0)
        self._ck(self.L.epv_dev_alloc(self.h, nbytes, C.byref(p)))
        return p

    def dev_free(self, p):
        self._ck(self.L.epv_dev_free(self.h, p))

    def run_mcmc_counts(self, burn_in, batch, seed, sweep_base=0):
        """run_mcmc of a shard: -> (the integer totals of its owned sites per batch sweep, int64
        [batch, 16 B]: J[8] then fixed-point D[8] per branch; accepted proposals).  Shards add
        their totals as integers; counts_to_stats turns the sum into J, D"""
        counts = np.zeros((batch, self.B * 16), np.int64)
        nacc = C.c_uint64(0)
        self._ck_mcmc(self.L.epv_run_mcmc_counts(self.h, burn_in, batch, seed, sweep_base,
                                                 _p(counts, C.c_int64), C.byref(nacc)))
        return counts, int(nacc.value)

    def counts_to_stats(self, counts, batch, average=True):
        c = np.ascontiguousarray(counts, np.int64)
        J, D = np.zeros(self.B * 8), np.zeros(self.B * 8)
        self._ck(self.L.epv_counts_to_stats(self.h, _p(c, C.c_int64), batch, int(average),
                                            _p(J, C.c_double), _p(D, C.c_double)))
        return J, D

    # ---- a genome sharded over several GPUs: device-resident halo columns and all-gather pieces
    # (buffers: DevBuf, or anything with .ptr = a device address on this context's GPU)
    def alloc(self, nbytes):
        return DevBuf(self, nbytes)

    def pack_columns(self, first, count, buf):
        self._ck(self.L.epv_pack_columns_dev(self.h, first, count, C.c_void_p(buf.ptr)))

    def unpack_columns(self, first, count, buf):
        self._ck(self.L.epv_unpack_columns_dev(self.h, first, count, C.c_void_p(buf.ptr)))

    def write(self, buf, offset, arr):
        a = np.ascontiguousarray(arr)
        self._ck(self.L.epv_dev_write(self.h, C.c_void_p(buf.ptr + offset), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def read(self, buf, offset, count, dtype=np.float64):
        out = np.zeros(count, dtype)
        self._ck(self.L.epv_dev_read(self.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(buf.ptr + offset), out.nbytes))
        return out

    def counters(self):
        c = _Counters()
        self._ck(self.L.epv_get_counters(self.h, C.byref(c)))
        return {"overflow": c.n_overflow, "coop_tasks": c.n_coop_tasks, "sweeps": c.n_sweeps,
                "search_finished": c.n_search_finished}

    def set_timing(self, on):
        self._ck(self.L.epv_set_timing(self.h, int(on)))

    def kernel_time_ms(self):
        ms, n = C.c_double(0), C.c_uint64(0)
        self._ck(self.L.epv_kernel_time_ms(self.h, C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    # ---- average history of the sampled paths (epv_set_path_average)
    def enable_path_average(self, n_points):
        """count the resident paths on a grid of n_points per branch after every batch sweep of
        run_mcmc (0 = off)"""
        self._ck(self.L.epv_set_path_average(self.h, int(n_points)))

    def path_average_layout(self):
        """(points, first local site, number of sites) of the counts; points = 0: averaging is off.
        A context counts its owned sites plus the genome's end sites when it holds them"""
        P, a, k = C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epv_path_average_layout(self.h, C.byref(P), C.byref(a), C.byref(k)))
        return int(P.value), int(a.value), int(k.value)

    def path_average(self, counts=False, chunk_bytes=256 << 20):
        """-> (samples, array [N-1, sites, P]): float64 averages, or the uint32 counts"""
        P, first, cnt = self.path_average_layout()
        if not P:
            raise EpvError(EPV_ERR_STATE, "path average is off: enable_path_average first")
        out = np.zeros((self.B, cnt, P), np.uint32)
        step = max(1, chunk_bytes // max(1, 4 * self.B * P))
        for a in range(0, cnt, step):
            k = min(step, cnt - a)
            buf = np.zeros((self.B, k, P), np.uint32)
            self._ck(self.L.epv_get_path_average(self.h, first + a, k, _p(buf, C.c_uint32)))
            out[:, a:a + k] = buf
        ns = self.path_average_samples()
        return ns, _per_sample(out, ns, counts)

    # ---- posterior branch-event maps (epv_set_branch_events)
    def enable_branch_events(self, on=True):
        """count end states, net and total gains and losses per (branch, site) after every batch sweep
        of run_mcmc (BRANCH_EVENT_PLANES; False = off)"""
        self._ck(self.L.epv_set_branch_events(self.h, 1 if on else 0))

    def branch_events_layout(self):
        """(first local site, number of sites) of the planes: the sites of path_average_layout"""
        a, k = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epv_branch_events_layout(self.h, C.byref(a), C.byref(k)))
        return int(a.value), int(k.value)

    def branch_events(self, counts=False):
        """-> (samples, array [6, N-1, sites]): float64 counts / samples, or the uint32 counts"""
        first, cnt = self.branch_events_layout()
        out = np.zeros((len(BRANCH_EVENT_PLANES), self.B, cnt), np.uint32)
        self._ck(self.L.epv_get_branch_events(self.h, first, cnt, _p(out, C.c_uint32)))
        ns = self.branch_events_samples()
        return ns, _per_sample(out, ns, counts)

    def branch_event_windows(self, W, first_window=0, n_windows=None):
        """-> (samples, uint64 [6, N-1, windows]): the planes summed over windows of W consecutive global
        sites, this context's contribution (zero where it counts no site); all windows of the genome
        unless a range is given"""
        W, n_windows = self._window_range(W, first_window, n_windows)
        out = np.zeros((len(BRANCH_EVENT_PLANES), self.B, n_windows), np.uint64)
        self._ck(self.L.epv_get_branch_event_windows(self.h, W, int(first_window), out.shape[2], _p(out, C.c_uint64)))
        return self.branch_events_samples(), out

    # ---- change patterns (epv_set_change_patterns)
    def enable_change_patterns(self, on=True):
        """count, per site, what happened across the branches of the tree -- the jump spectrum, one-branch,
        parallel and reverted changes, sole gains and losses per branch, changed clades -- after every batch
        sweep of run_mcmc (CHANGE_PATTERN_ROWS; False = off)"""
        self._ck(self.L.epv_set_change_patterns(self.h, 1 if on else 0))

    def change_patterns_layout(self):
        """(rows R, clade nodes [I], first local site, number of sites): R = 12 + 2 (N-1) + I, the clade nodes
        are the internal non-root nodes in pre-order; (0, [], 0, 0) when off"""
        R, I, a, k = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        nodes = np.zeros(max(self.B, 1), np.uint32)
        self._ck(self.L.epv_change_patterns_layout(self.h, C.byref(R), C.byref(I), _p(nodes, C.c_uint32), C.byref(a),
                                                   C.byref(k)))
        return int(R.value), nodes[:I.value].copy(), int(a.value), int(k.value)

    def change_patterns(self, counts=False):
        """-> (samples, array [R, sites]): float64 counts / samples, or the uint32 counts"""
        R, _, first, cnt = self.change_patterns_layout()
        out = np.zeros((R, cnt), np.uint32)
        self._ck(self.L.epv_get_change_patterns(self.h, first, cnt, _p(out, C.c_uint32)))
        ns = self.change_patterns_samples()
        return ns, _per_sample(out, ns, counts)

    def change_pattern_windows(self, W, first_window=0, n_windows=None):
        """-> (samples, uint64 [R, windows]): the rows summed over windows of W consecutive global sites, this
        context's contribution (zero where it counts no site); all windows of the genome unless a range is given"""
        W, n_windows = self._window_range(W, first_window, n_windows)
        out = np.zeros((self.change_patterns_layout()[0], n_windows), np.uint64)
        self._ck(self.L.epv_get_change_pattern_windows(self.h, W, int(first_window), out.shape[1], _p(out, C.c_uint64)))
        return self.change_patterns_samples(), out

    # ---- regional sufficient statistics (epv_set_window_stats)
    def enable_window_stats(self, W):
        """add J and D per window of W global sites after every batch sweep of run_mcmc (0 = off)"""
        W = int(W)
        if W < 0:
            raise ValueError("a window holds at least one site (0 turns the statistics off)")
        self._ck(self.L.epv_set_window_stats(self.h, W))

    def window_stats_layout(self):
        """(W as clamped, first global window, number of windows) this context holds; (0, 0, 0) when off"""
        w, a, k = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epv_window_stats_layout(self.h, C.byref(w), C.byref(a), C.byref(k)))
        return int(w.value), int(a.value), int(k.value)

    def window_stats_scale_exps(self):
        """k_b of the non-root nodes: a D integer of the accumulator is a dwell time in units of 2^-k_b"""
        k = np.zeros(max(self.B, 1), np.intc)
        self._ck(self.L.epv_window_stats_scale_exps(self.h, _p(k, C.c_int)))
        return k[:self.B]

    def window_counts(self, first_window=0, n_windows=None):
        """-> (samples, int64 [windows, N-1, 16]): this context's contribution (J[8] then D[8] as integers),
        zero where it holds no site; all windows of the genome unless a range is given"""
        W = self.window_stats_layout()[0]
        if not W:
            self._ck(self.L.epv_get_window_stats(self.h, 0, 0, None))     # off: EPV_ERR_STATE
        out = np.zeros((self._window_range(W, first_window, n_windows)[1], self.B, 16), np.int64)
        self._ck(self.L.epv_get_window_stats(self.h, int(first_window), out.shape[0], _p(out, C.c_int64)))
        return self.window_stats_samples(), out

    def window_counts_to_stats(self, counts, samples):
        """int64 [windows, N-1, 16] -> J, D [windows, N-1, 8] per sample (D in time units)"""
        counts = np.ascontiguousarray(counts, np.int64)
        J, D = np.zeros(counts.shape[:2] + (8,)), np.zeros(counts.shape[:2] + (8,))
        if counts.shape[0]:
            self._ck(self.L.epv_window_counts_to_stats(self.h, _p(counts, C.c_int64), counts.shape[0], int(samples),
                                                       _p(J, C.c_double), _p(D, C.c_double)))
        return J, D

    def window_stats(self, counts=False):
        """-> (samples, J[nw, N-1, 8], D[nw, N-1, 8]) averaged over the samples, or (samples, int64
        [nw, N-1, 16]) with counts=True"""
        ns, cnt = self.window_counts()
        if counts:
            return ns, cnt
        if not ns:
            raise RuntimeError("window statistics hold no sample")
        return (ns,) + self.window_counts_to_stats(cnt, ns)

    # ---- lineage origin maps (epv_set_lineage_origins)
    def enable_lineage_origins(self, on=True):
        """count, per leaf and site, on which branch of the leaf's lineage the sampled history last changed
        state, and the age of the leaf's state, after every batch sweep of run_mcmc (False = off)"""
        self._ck(self.L.epv_set_lineage_origins(self.h, 1 if on else 0))

    def lineage_origins_layout(self):
        """(leaves L, rows R, first local site, number of sites); zeros when off"""
        nl, nr, a, k = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epv_lineage_origins_layout(self.h, C.byref(nl), C.byref(nr), C.byref(a), C.byref(k)))
        return int(nl.value), int(nr.value), int(a.value), int(k.value)

    def lineage_origin_rows(self):
        """uint32 [R, 2]: per row the leaf node and the branch node (0 = the leaf's root row)"""
        R = self.lineage_origins_layout()[1]
        leaf, node = np.zeros(max(R, 1), np.uint32), np.zeros(max(R, 1), np.uint32)
        self._ck(self.L.epv_lineage_origin_rows(self.h, _p(leaf, C.c_uint32), _p(node, C.c_uint32)))
        return np.stack([leaf[:R], node[:R]], axis=1)

    def lineage_origins_scale_exp(self):
        """k: an age integer is a time in units of 2^-k"""
        k = C.c_int(0)
        self._ck(self.L.epv_lineage_origins_scale_exp(self.h, C.byref(k)))
        return int(k.value)

    def lineage_origins(self, counts=False):
        """-> (samples, rows [R, 2], origin [R, sites], age [L, sites]): origin / samples = the posterior over the
        origin branch per leaf and site, age * 2^-k / samples = the posterior mean age of the leaf's state
        in branch-length units; counts=True gives the uint32 and uint64 sums"""
        rows = self.lineage_origin_rows()
        L, R, first, cnt = self.lineage_origins_layout()
        origin, age = np.zeros((R, cnt), np.uint32), np.zeros((L, cnt), np.uint64)
        self._ck(self.L.epv_get_lineage_origins(self.h, first, cnt, _p(origin, C.c_uint32), _p(age, C.c_uint64)))
        ns = self.lineage_origins_samples()
        if counts:
            return ns, rows, origin, age
        k = self.lineage_origins_scale_exp()
        d = float(ns) if ns else 1.0
        return ns, rows, origin / d, np.ldexp(age.astype(np.float64), -k) / d

    def lineage_origin_windows(self, W, first_window=0, n_windows=None):
        """-> (samples, uint64 [R, windows], uint64 [L, windows]): the origin rows and the ages summed over
        windows of W consecutive global sites, this context's contribution (zero where it counts no site);
        all windows of the genome unless a range is given"""
        W, n_windows = self._window_range(W, first_window, n_windows)
        L, R = self.lineage_origins_layout()[:2]
        out = np.zeros((R + L, n_windows), np.uint64)
        self._ck(self.L.epv_get_lineage_origin_windows(self.h, W, int(first_window), out.shape[1], _p(out, C.c_uint64)))
        return self.lineage_origins_samples(), out[:R], out[R:]


    # ---- domain size spectra (epv_set_domain_stats)
    def enable_domain_stats(self, max_samples):
        """count the run lengths of every node's state along the genome after every batch sweep of run_mcmc, for
        at most max_samples samples (0 = off)"""
        self._ck(self.L.epv_set_domain_stats(self.h, int(max_samples)))

    def domain_stats_layout(self):
        """(nodes N, bins, first local site, number of sites, sites per block of the runs kernel); zeros when off"""
        nn, nb, a, k, cs = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epv_domain_stats_layout(self.h, C.byref(nn), C.byref(nb), C.byref(a), C.byref(k), C.byref(cs)))
        return int(nn.value), int(nb.value), int(a.value), int(k.value), int(cs.value)

    def domain_stats_part(self):
        """-> (samples, hist [N, 2, 128], len_sum [N, 2], edges [samples, N, 2]), uint64: what this context's
        stretch of sites contributes, unclosed (host.domain_parts_merge, host.domain_part_close)"""
        ns = self.domain_stats_samples()
        N, nb = self.domain_stats_layout()[:2]
        hist, len_sum = np.zeros((max(N, 1), 2, max(nb, 1)), np.uint64), np.zeros((max(N, 1), 2), np.uint64)
        edges = np.zeros((max(ns, 1), max(N, 1), 2), np.uint64)
        self._ck(self.L.epv_get_domain_stats(self.h, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64), _p(edges, C.c_uint64)))
        return ns, hist[:N], len_sum[:N], edges[:ns, :N]

    def domain_stats(self):
        """-> (samples, hist [N, 2, 128], len_sum [N, 2]): the closed result over this context's sites.  hist /
        samples is the posterior spectrum of run lengths per node and state; the runs at the two ends count with
        the length the stretch leaves them"""
        ns, hist, len_sum, edges = self.domain_stats_part()
        return (ns,) + host.domain_part_close(hist, len_sum, edges)

    # ---- domain turnover (epv_set_domain_turnover)
    def enable_domain_turnover(self, max_samples):
        """count, per branch, the runs of the state at its start and at its end along the genome, each kept or
        turned over, after every batch sweep of run_mcmc, for at most max_samples samples (0 = off)"""
        self._ck(self.L.epv_set_domain_turnover(self.h, int(max_samples)))

    def domain_turnover_layout(self):
        """(rows R = 2 B, bins, first local site, number of sites, sites per block of the runs kernel); zeros when off"""
        nr, nb, a, k, cs = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epv_domain_turnover_layout(self.h, C.byref(nr), C.byref(nb), C.byref(a), C.byref(k), C.byref(cs)))
        return int(nr.value), int(nb.value), int(a.value), int(k.value), int(cs.value)

    def domain_turnover_part(self):
        """-> (samples, hist [R, 2, 2, 128], len_sum [R, 2, 2], edges [samples, R, 2]), uint64: what this context's
        stretch of sites contributes, unclosed (host.turnover_parts_merge, host.turnover_part_close)"""
        ns = self.domain_turnover_samples()
        R, nb = self.domain_turnover_layout()[:2]
        hist = np.zeros((max(R, 1), 2, 2, max(nb, 1)), np.uint64)
        len_sum = np.zeros((max(R, 1), 2, 2), np.uint64)
        edges = np.zeros((max(ns, 1), max(R, 1), 2), np.uint64)
        self._ck(self.L.epv_get_domain_turnover(self.h, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64),
                                                _p(edges, C.c_uint64)))
        return ns, hist[:R], len_sum[:R], edges[:ns, :R]

    def domain_turnover(self):
        """-> (samples, hist [R, 2, 2, 128], len_sum [R, 2, 2]): the closed result over this context's sites; row
        2 b is the start of branch b, row 2 b + 1 its end; axes state and kept (host.domain_turnover_summary)"""
        ns, hist, len_sum, edges = self.domain_turnover_part()
        return (ns,) + host.turnover_part_close(hist, len_sum, edges)

    # ---- change tracts (epv_set_change_tracts)
    def enable_change_tracts(self, max_samples):
        """count, per branch, the maximal runs of sites with a net change (tracts) by direction (gain, loss, mixed),
        by the state of the unchanged site on each flank and by length, after every batch sweep of run_mcmc, for at
        most max_samples samples (0 = off)"""
        self._ck(self.L.epv_set_change_tracts(self.h, int(max_samples)))

    def change_tracts_layout(self):
        """(branches B, classes, bins, first local site, number of sites, sites per block of the tract kernel); zeros
        when off"""
        nb, nc, nbin, a, k, cs = (C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0),
                                  C.c_uint64(0))
        self._ck(self.L.epv_change_tracts_layout(self.h, C.byref(nb), C.byref(nc), C.byref(nbin), C.byref(a), C.byref(k),
                                                 C.byref(cs)))
        return int(nb.value), int(nc.value), int(nbin.value), int(a.value), int(k.value), int(cs.value)

    def change_tracts_part(self):
        """-> (samples, hist [B, 27, 128], len_sum [B, 27], edges [samples, B, 2]), uint64: what this context's
        stretch of sites contributes, unclosed (host.tract_parts_merge, host.tract_part_close)"""
        ns = self.change_tracts_samples()
        B, nc, nb = self.change_tracts_layout()[:3]
        nc = nc or host.TRACT_CLASSES
        hist = np.zeros((max(B, 1), nc, max(nb, 1)), np.uint64)
        len_sum = np.zeros((max(B, 1), nc), np.uint64)
        edges = np.zeros((max(ns, 1), max(B, 1), 2), np.uint64)
        self._ck(self.L.epv_get_change_tracts(self.h, _p(hist, C.c_uint64), _p(len_sum, C.c_uint64), _p(edges, C.c_uint64)))
        return ns, hist[:B], len_sum[:B], edges[:ns, :B]

    def change_tracts(self):
        """-> (samples, hist [B, 27, 128], len_sum [B, 27]): the closed result over this context's sites; class =
        direction * 9 + left * 3 + right (host.change_tract_summary)"""
        ns, hist, len_sum, edges = self.change_tracts_part()
        return (ns,) + host.tract_part_close(hist, len_sum, edges)

    # ---- spatial correlations (epv_set_spatial_correlation)
    def enable_spatial_correlation(self, max_lag, max_samples):
        """count, per node state row and branch change row, the site pairs (p, p + d) that are both 1 for every lag
        d = 0 .. max_lag (at most 1024) after every batch sweep of run_mcmc, for at most max_samples samples
        (max_lag = 0: off)"""
        self._ck(self.L.epv_set_spatial_correlation(self.h, int(max_lag), int(max_samples)))

    def spatial_correlation_layout(self):
        """(rows R = N + B, max_lag, first local site, number of sites, sites per block of the count kernel); zeros
        when off"""
        nr, ml, a, k, cs = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epv_spatial_correlation_layout(self.h, C.byref(nr), C.byref(ml), C.byref(a), C.byref(k),
                                                       C.byref(cs)))
        return int(nr.value), int(ml.value), int(a.value), int(k.value), int(cs.value)

    def spatial_correlation_part(self):
        """-> (samples, sites, n11 [R, L + 1], edges [samples, R, 2, ceil(L / 64)]), uint64: what this context's
        stretch of sites contributes, unclosed (host.corr_parts_merge, host.corr_part_close)"""
        ns = self.spatial_correlation_samples()
        R, L, _, cnt, _ = self.spatial_correlation_layout()
        LW = (L + 63) // 64
        n11 = np.zeros((max(R, 1), L + 1), np.uint64)
        edges = np.zeros(max(ns * R * 2 * LW, 1), np.uint64)
        self._ck(self.L.epv_get_spatial_correlation(self.h, _p(n11, C.c_uint64), _p(edges, C.c_uint64)))
        return ns, cnt, n11[:R], edges[:ns * R * 2 * LW].reshape(ns, R, 2, LW)

    def spatial_correlation(self):
        """-> (samples, n11, left1, right1), each [R, L + 1]: the closed result over this context's sites; rows 0 ..
        N - 1 the node states, rows N .. N + B - 1 the net changes of the branches (host.spatial_correlation_summary)"""
        ns, cnt, n11, edges = self.spatial_correlation_part()
        return (ns,) + host.corr_part_close(cnt, n11, edges)

    # ---- domain maps (epv_set_domain_maps)
    def enable_domain_maps(self, sizes, state=1, max_samples=1 << 21):
        """count, per node, size and site, the samples in which the site lies in a run of `state` of at least that
        size along the genome, after every batch sweep of run_mcmc, for at most max_samples samples: 1 .. 4 strictly
        increasing sizes of 1 .. 1024 (an empty list: off)"""
        z = np.array([int(L) for L in np.atleast_1d(sizes)], np.uint32) if np.size(sizes) else np.zeros(0, np.uint32)
        if not len(z):
            return self._ck(self.L.epv_set_domain_maps(self.h, 0, None, 0, 0))
        z = host.domain_map_sizes(z)
        if int(state) not in (0, 1):
            raise ValueError("the state of the domain maps is 0 or 1")
        self._ck(self.L.epv_set_domain_maps(self.h, len(z), _p(z, C.c_uint32), int(state), int(max_samples)))

    def domain_maps_layout(self):
        """(nodes N, sizes tuple, state, first local site, number of sites, sites per block of the membership kernel);
        (0, (), 0, 0, 0, 0) when off"""
        nn, nk, st = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        z = np.zeros(4, np.uint32)
        a, k, cs = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.epv_domain_maps_layout(self.h, C.byref(nn), C.byref(nk), _p(z, C.c_uint32), C.byref(st),
                                               C.byref(a), C.byref(k), C.byref(cs)))
        return (int(nn.value), tuple(int(L) for L in z[:int(nk.value)]), int(st.value), int(a.value), int(k.value),
                int(cs.value))

    def domain_maps_part(self):
        """-> (samples, sites, counts uint32 [N, K, sites], edges uint64 [samples, N, 2, EW]): what this context's
        stretch of sites contributes, unmerged (host.domain_maps_merge); EW = ceil((L_K - 1) / 32)"""
        ns = self.domain_maps_samples()
        N, z, _, _, cnt, _ = self.domain_maps_layout()
        K = len(z)
        EW = (2 * (z[-1] - 1) + 63) // 64 if K else 0
        counts = np.zeros(max(N * K * cnt, 1), np.uint32)
        edges = np.zeros(max(ns * N * 2 * EW, 1), np.uint64)
        self._ck(self.L.epv_get_domain_maps(self.h, _p(counts, C.c_uint32), _p(edges, C.c_uint64)))
        return ns, cnt, counts[:N * K * cnt].reshape(N, K, cnt), edges[:ns * N * 2 * EW].reshape(ns, N, 2, EW)

    def domain_maps(self, counts=False):
        """-> (samples, maps [N, K, sites]): maps[v, k, p] = the posterior probability that site p of node v lies in
        a run of the state asked for of at least sizes[k] sites (over this context's sites); counts=True gives the
        uint32 counts (host.domain_calls, host.domain_map_windows)"""
        ns, _, c, _ = self.domain_maps_part()
        return ns, _per_sample(c, ns, counts)

    # ---- epoch statistics (epv_set_epoch_stats)
    def enable_epoch_stats(self, P):
        """add J and D per branch and epoch (P epochs per branch) after every batch sweep of run_mcmc (0 = off)"""
        P = int(P)
        if P < 0 or P > EPOCH_MAX_P:
            raise ValueError("1 .. %d epochs per branch (0 turns the statistics off)" % EPOCH_MAX_P)
        self._ck(self.L.epv_set_epoch_stats(self.h, P))

    def epoch_stats_layout(self):
        """(P, k_b int[N-1], fixT_b uint64[N-1]) of the accumulator's samples; (0, [], []) when off"""
        B, P = C.c_uint32(0), C.c_uint32(0)
        k, f = np.zeros(max(self.B, 1), np.intc), np.zeros(max(self.B, 1), np.uint64)
        self._ck(self.L.epv_epoch_stats_layout(self.h, C.byref(B), C.byref(P), _p(k, C.c_int), _p(f, C.c_uint64)))
        return int(P.value), k[:int(B.value)], f[:int(B.value)]

    def epoch_raw(self):
        """-> (samples, uint64 [N-1, P, 32]): this context's raw part (J[8], lo[8], hi[8], cov[8]); raw parts
        of the contexts of a genome add up (host.epoch_raw_add) and are closed once (host.epoch_close)"""
        P = self.epoch_stats_layout()[0]
        if not P:
            self._ck(self.L.epv_get_epoch_stats(self.h, None))     # off: EPV_ERR_STATE
        out = np.zeros((self.B, P, 32), np.uint64)
        self._ck(self.L.epv_get_epoch_stats(self.h, _p(out, C.c_uint64)))
        return self.epoch_stats_samples(), out

    def epoch_stats(self, counts=False):
        """-> (samples, J[N-1, P, 8], D[N-1, P, 8]) averaged over the samples (D in time units), or with
        counts=True the closed integers: J int64, D Python ints (object array) in units of 2^-k_b"""
        ns, raw = self.epoch_raw()
        _, k, fixT = self.epoch_stats_layout()
        return host.epoch_finish(raw, fixT, k, ns, counts)

    # ---- chain mixing diagnostics (epv_set_mixing)
    def enable_mixing(self, max_lag=8):
        """count, per site, the linked sample pairs whose history differs, and the sums of the site's jump count x
        and of its lagged products up to max_lag (1 .. MIXING_MAX_LAG) after every batch sweep of run_mcmc, the state
        after burn-in as the opening state of the run (0 = off)"""
        self._ck(self.L.epv_set_mixing(self.h, int(max_lag)))

    def mixing_layout(self):
        """(first local site, number of sites, max_lag): the sites of path_average_layout; zeros when off"""
        a, k, ml = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        self._ck(self.L.epv_mixing_layout(self.h, C.byref(a), C.byref(k), C.byref(ml)))
        return int(a.value), int(k.value), int(ml.value)

    def mixing(self, counts=False):
        """counts=True -> (samples, moved_pairs, pairs uint64[K + 1] (pairs[k] at lag k, pairs[0] = 0), moved
        uint32[sites], S1 uint64[sites], S2 uint64[sites], C uint64[K, sites]); otherwise the dict
        host.mixing_summary makes of them"""
        first, cnt, K = self.mixing_layout()
        words = np.zeros(MIXING_MAX_LAG + 2, np.uint64)
        self._ck(self.L.epv_mixing_pairs(self.h, _p(words, C.c_uint64)))
        moved, sums = np.zeros(cnt, np.uint32), np.zeros((2 + K, cnt), np.uint64)
        self._ck(self.L.epv_mixing_counts(self.h, first, cnt, _p(moved, C.c_uint32), _p(sums, C.c_uint64)))
        pairs = np.concatenate([np.zeros(1, np.uint64), words[2:2 + K]])
        out = (int(words[0]), int(words[1]), pairs, moved, sums[0], sums[1], sums[2:])
        return out if counts else host.mixing_summary(*out)

    def mixing_windows(self, W, first_window=0, n_windows=None):
        """-> (samples, moved_pairs, uint64 [windows]): moved summed over windows of W consecutive global sites, this
        context's contribution (zero where it counts no site); all windows of the genome unless a range is given"""
        W, n_windows = self._window_range(W, first_window, n_windows)
        out = np.zeros(n_windows, np.uint64)
        words = np.zeros(MIXING_MAX_LAG + 2, np.uint64)
        self._ck(self.L.epv_mixing_pairs(self.h, _p(words, C.c_uint64)))
        self._ck(self.L.epv_mixing_windows(self.h, W, int(first_window), n_windows, _p(out, C.c_uint64)))
        return int(words[0]), int(words[1]), out


for _s in CHAIN:
    setattr(DeviceSampler, "reset_" + _s.stem, summary_method(DeviceSampler._reset_summary, _s, "reset_" + _s.stem))
    setattr(DeviceSampler, "accumulate_" + _s.stem,
            summary_method(DeviceSampler._accumulate_summary, _s, "accumulate_" + _s.stem,
                           "the resident paths as one more sample (for callers that drive sweep() themselves)"))
    setattr(DeviceSampler, _s.stem + "_samples",
            summary_method(DeviceSampler._summary_samples, _s, _s.stem + "_samples"))


def forward_to_dev(cls, names):
    """give cls the methods `names` of DeviceSampler, each forwarding to self.dev (resolved by name at call time: a
    LocalGroup or a test's stand-in serves as well) under DeviceSampler's signature and docstring"""
    def make(name):
        @functools.wraps(getattr(DeviceSampler, name))
        def method(self, *args, **kwargs):
            return getattr(self.dev, name)(*args, **kwargs)
        return method
    for name in names:
        setattr(cls, name, make(name))


class SingleSiteSampler:
    """Mirror of the reference class (SingleSiteSampler.hpp:35-81).

    mcmc = SingleSiteSampler(burn_in, batch); mcmc.reset(model, tree, paths);
    J, D, acc_rate = mcmc.run_mcmc(seed, em_iter)      # paths stay on the GPU
    paths = mcmc.paths()                               # download when needed
    The reference threads one std::mt19937 through every call; here the random
    stream is the counter-based (seed, sweep) pair, so the caller passes the seed and
    the index of the EM iteration (sweep numbers never repeat across iterations)."""

    def __init__(self, n_burn_in, n_batch, device=0, capacity=0, direct_sampler=False, direct_fused=False, leaf_fast=False):
        self.burn_in, self.batch = int(n_burn_in), int(n_batch)
        # hard-wired false in the reference (SingleSiteSampler.cpp:441) and set by none of its programs;
        # True = EPV_OPT_SAMPLE_ROOT: root states are proposed too (reference-arithmetic kernels)
        self.SAMPLE_ROOT = False
        # True = EPV_OPT_DIRECT_SAMPLER: jump times in bounded work per segment (no reference counterpart)
        self.direct_sampler = bool(direct_sampler)
        # with direct_sampler: EPV_OPT_DIRECT_FUSED, the fused phase's direct bodies where the fused phase is eligible
        self.direct_fused = bool(direct_fused)
        # True = EPV_OPT_LEAF_FAST: held leaf cells keep the fused / second / third proposal kernels (leaf variants)
        self.leaf_fast = bool(leaf_fast)
        self.capacity = capacity
        self.dev = DeviceSampler(device)
        self.dev.auto_grow = True     # paths grow on demand, as the reference's vectors do
        self._uploaded = False
        self._unobserved = None       # the mask of unobserved leaf cells, re-applied after every upload
        self._leaf_evidence = None    # the table of leaf evidence, likewise
        self._regions = None          # the lengths of the genomic regions, likewise (their end sites are held fixed)

    def _apply_sample_root(self):
        flags = C.c_uint32(0)
        self.dev._ck(self.dev.L.epv_get_options(self.dev.h, C.byref(flags)))
        want = (flags.value | 4) if self.SAMPLE_ROOT else (flags.value & ~4)
        want = (want & ~24) | ((8 | (16 if self.direct_fused else 0)) if self.direct_sampler else 0)
        want = (want & ~32) | (32 if self.leaf_fast else 0)
        if want != flags.value:
            self.dev._ck(self.dev.L.epv_set_options(self.dev.h, want))

    def reset(self, model, tree, paths=None):
        self.dev.set_tree(tree)
        self.dev.set_model(model)
        if paths is not None:
            self.dev.upload_paths(paths, self.capacity)
            self._uploaded = True
            if self._unobserved is not None:
                self.dev.set_unobserved(self._unobserved)
            if self._leaf_evidence is not None:
                self.dev.set_leaf_evidence(self._leaf_evidence)
            if self._regions is not None:
                self.dev.set_fixed_sites(host.region_fixed_mask(paths.n_sites, self._regions))
        if not self._uploaded:
            raise EpvError(EPV_ERR_STATE, "reset() needs paths the first time")
        self._apply_sample_root()
        self.dev.reset()

    def set_unobserved(self, mask):
        """missing leaf data (DeviceSampler.set_unobserved); kept across resets, re-applied to new paths.
        None clears."""
        if mask is None:
            self._unobserved = None
        else:
            self._unobserved = (np.ascontiguousarray(mask).reshape(-1) != 0).astype(np.uint8)
        if self._uploaded:
            self.dev.set_unobserved(self._unobserved)

    def set_leaf_evidence(self, p_state1):
        """leaf evidence (DeviceSampler.set_leaf_evidence); kept across resets, re-applied to new paths.
        None clears."""
        if p_state1 is None:
            self._leaf_evidence = None
        else:
            self._leaf_evidence = np.ascontiguousarray(p_state1, np.float32).reshape(-1).copy()
        if self._uploaded:
            self.dev.set_leaf_evidence(self._leaf_evidence)

    def set_regions(self, lengths):
        """genomic regions (chromosomes, gap-free stretches): their numbers of sites in the order of the paths, each
        at least 3, summing to the number of sites (host.read_regions reads them from a file).  The first and the
        last site of every region are held fixed (DeviceSampler.set_fixed_sites), so no triple and no update spans a
        break: the regions are sampled and counted independently given their end columns.  Kept across resets,
        re-applied to new paths.  None clears."""
        self._regions = None if lengths is None else [int(m) for m in lengths]
        if self._uploaded:
            self.dev.set_fixed_sites(None if self._regions is None
                                     else host.region_fixed_mask(self.dev.n_sites, self._regions))

    def run_mcmc(self, seed, em_iter=0):
        self._apply_sample_root()
        base = em_iter * (self.burn_in + self.batch)
        J, D, nacc = self.dev.run_mcmc(self.burn_in, self.batch, seed, base)
        updatable = self.dev.n_sites - 2 - (self.dev.fixed_sites() if self._regions is not None else 0)
        acc_rate = nacc / float(self.batch * updatable)
        return J, D, acc_rate

    def sweeps(self, n, seed, sweep_base=0):
        self._apply_sample_root()
        return self.dev.sweep(n, seed, sweep_base)


# everything else is DeviceSampler's: the four lifecycle methods of every summary, and
forward_to_dev(SingleSiteSampler, LIFECYCLE + [
    "scale_jump_times", "paths", "path_average", "branch_events", "branch_event_windows", "window_stats", "epoch_stats",
    "lineage_origins_layout", "lineage_origin_rows", "lineage_origins_scale_exp", "lineage_origins",
    "lineage_origin_windows", "domain_stats_layout", "domain_stats_part", "domain_stats", "change_patterns_layout",
    "change_patterns", "change_pattern_windows", "domain_turnover_layout", "domain_turnover_part", "domain_turnover",
    "spatial_correlation_layout", "spatial_correlation_part", "spatial_correlation", "mixing_layout", "mixing",
    "mixing_windows", "domain_maps_layout", "domain_maps_part", "domain_maps", "change_tracts_layout",
    "change_tracts_part", "change_tracts"])
