"""The posterior summaries run_mcmc can take, as the Python layers above the device see them (DESIGN.md section
7.15): one table, and the few rules that are the same for every summary and every layer."""
from collections import namedtuple

import numpy as np

# stem: epv_set_<stem>, epv_reset_<stem>, epv_accumulate_<stem>, epv_<stem>_samples in the C ABI and enable_<stem>,
# reset_<stem>, accumulate_<stem>, <stem>_samples on every sampler; article, noun: "... taking a path-average
# sample", "... different numbers of path-average samples".  The order is that of kLayers in epv_abi.hip
Summary = namedtuple("Summary", "stem article noun")
SUMMARIES = (
    Summary("path_average", "a", "path-average"),
    Summary("branch_events", "a", "branch-event"),
    Summary("window_stats", "a", "window-statistics"),
    Summary("epoch_stats", "an", "epoch-statistics"),
    Summary("lineage_origins", "a", "lineage-origin"),
    Summary("domain_stats", "a", "domain-statistics"),
    Summary("change_patterns", "a", "change-pattern"),
    Summary("domain_turnover", "a", "domain-turnover"),
    Summary("spatial_correlation", "a", "spatial-correlation"),
)
# what run_mcmc can take besides: diagnostics of the chain itself, the same record and the same lifecycle.  After
# SUMMARIES in kLayers
DIAGNOSTICS = (
    Summary("mixing", "a", "mixing"),
)
# summaries that joined the chain after the diagnostics: after DIAGNOSTICS in kLayers, so that every order the two
# tables above stand for stays what it was
LATER_SUMMARIES = (
    Summary("domain_maps", "a", "domain-map"),
)
LAYERS = SUMMARIES + DIAGNOSTICS + LATER_SUMMARIES
# summaries that joined the chain after those: a fourth table, because the three above and their sum LAYERS are
# what they were when tests recorded them.  CHAIN is every entry of kLayers in its order; what loops over "every
# layer" loops over CHAIN
TRACT_SUMMARIES = (
    Summary("change_tracts", "a", "change-tract"),
)
CHAIN = LAYERS + TRACT_SUMMARIES
NOUN = {s.stem: s.noun for s in CHAIN}
# the four methods every sampler has for every summary and diagnostic
LIFECYCLE = [fmt % s.stem for s in CHAIN for fmt in ("enable_%s", "reset_%s", "accumulate_%s", "%s_samples")]


def summary_method(helper, row, name, doc=None):
    """the method `name` of a summary: helper(self, row), the row of SUMMARIES bound"""
    def method(self):
        return helper(self, row)
    method.__name__, method.__qualname__, method.__doc__ = name, name, doc
    return method


def _per_sample(out, ns, counts):
    """the tail of a read-out of counts: the integers as they are, or float64 counts / samples (the zeros of an
    accumulator without a sample stay zeros)"""
    return out if counts else out / float(ns) if ns else out.astype(np.float64)


def _window_range(W, n_sites, first_window, n_windows):
    """-> (W, number of windows): windows of W consecutive global sites from first_window on, all the rest of a genome
    of n_sites unless n_windows says how many"""
    W = int(W)
    if W < 1:
        raise ValueError("a window holds at least one site")
    if n_windows is None:
        n_windows = (n_sites + W - 1) // W - first_window
    return W, max(int(n_windows), 0)
