"""The reference of genomic regions: every region run ALONE through the parity oracle's
parallel rung B, with the random keys of its place in the genome; the whole-genome result is the concatenated paths,
the summed integer rows per sweep and the summed accept counts.

Region [a, a + m) of a genome of n sites:
  * its first and last site are never resampled, they are context for their inner neighbour, and they centre no
    counted triple;
  * a sweep w is orc_sweep_phase(h, c, w, first, last, first, last) for c = 0, 1, 2 over its inner sites
    a + 1 .. a + m - 2, the integer statistics orc_suffstats_rows over the same centres (as
    tests/test_exact_stats.py::_rows).

The oracle is built on the region's columns PLUS the one column next to each end where the genome goes on (the
neighbouring region's end site, fixed like this region's own, so a constant of the chain), and orc_set_shard gives
it the global index of its column 0.  That context column is needed: the acceptance of the first inner site a + 1
reads the cached likelihood of the triple centred at the fixed site a whenever a is not the genome's own first
site (mh_site: g0 + site > 1), and that triple's left column is a - 1; the same at the other end.  An oracle
built on [a, a + m) alone with g0 = a would read the column before its first one there.  So what a region run
alone needs of the rest of the genome is those two fixed columns and nothing else: given the end columns the
regions are independent, and test_regions.py pins that this equals the whole-genome oracle stepped over the
non-fixed sites only.
"""
import ctypes as C

import numpy as np

import orc
from epievo_amd.parallel import concat_sites


def region_starts(lengths):
    return [int(x) for x in np.cumsum([0] + list(lengths[:-1]))]


class RegionsRef:
    """opts: the keywords of DeviceSampler.set_options; unobserved / evidence: [B, n] as the device takes them"""

    def __init__(self, tree, model, fp, lengths, cap, seed, opts=None, unobserved=None, evidence=None):
        opts = opts or {}
        n = fp.n_sites
        assert sum(lengths) == n and min(lengths) >= 3
        self.n, self.B, self.lengths = n, tree.n_nodes - 1, list(lengths)
        self.regions = []
        for a, m in zip(region_starts(lengths), lengths):
            lo, hi = (a - 1 if a > 0 else a), (a + m + 1 if a + m < n else a + m)
            o = orc.Oracle(tree, model, fp.slice_sites(lo, hi), "B", cap=cap, seed=seed)
            o.set_sampler(bool(opts.get("forward_rejection")))
            o.set_proposal_mode(bool(opts.get("reference_proposal_ratio")))
            o.set_sample_root(bool(opts.get("sample_root")))
            if unobserved is not None:
                o.set_unobserved(np.asarray(unobserved).reshape(self.B, n)[:, lo:hi])
            if evidence is not None:
                o.set_leaf_evidence(np.asarray(evidence, np.float32).reshape(self.B, n)[:, lo:hi])
            o.L.orc_set_shard(o.h, lo, n)
            self.regions.append((o, a - lo, m))
        self.reset()

    def reset(self):
        for o, _, _ in self.regions:
            o.reset()

    def sweep(self, w):
        """one sweep of every region -> accepted proposals"""
        nacc = 0
        for o, off, m in self.regions:
            first, last = off + 1, off + m - 2
            for c in range(3):
                nacc += int(o.L.orc_sweep_phase(o.h, c, w, first, last, first, last))
        return nacc

    def region_counts(self):
        """int64 [regions, B, 16]: the integer J and D of every region's inner centres"""
        out = np.zeros((len(self.regions), self.B, 16), np.int64)
        for k, (o, off, m) in enumerate(self.regions):
            one = np.zeros((1, self.B, 16), np.int64)
            o.L.orc_suffstats_rows(o.h, 0, o.n_sites, 1, off + 1, off + m - 2, orc._p(one, C.c_int64))
            out[k] = one[0]
        return out

    def run_mcmc_counts(self, burn_in, batch, sweep_base=0):
        """as DeviceSampler.run_mcmc_counts -> (int64 [batch, B * 16], accepted proposals of the batch sweeps)"""
        w = sweep_base
        for _ in range(burn_in):
            self.sweep(w)
            w += 1
        counts, nacc = np.zeros((batch, self.B * 16), np.int64), 0
        for i in range(batch):
            nacc += self.sweep(w)
            w += 1
            counts[i] = self.region_counts().sum(axis=0).reshape(-1)
        return counts, nacc

    def paths(self):
        return concat_sites([o.paths().slice_sites(off, off + m) for o, off, m in self.regions])

    def region_paths(self):
        return [o.paths().slice_sites(off, off + m) for o, off, m in self.regions]

    def tri_llh(self):
        return np.concatenate([o.tri_llh()[off:off + m] for o, off, m in self.regions])

    def overflow(self):
        return sum(o.counters()["overflow"] for o, _, _ in self.regions)


def whole_genome_paths(tree, model, fp, lengths, cap, seed, sweeps, sweep_base=0, opts=None):
    """the other formulation of the same chain: ONE rung-B oracle over the whole genome (g0 = 0), stepped colour by
    colour with orc_mh_site over the non-fixed sites only -> (paths, accepted proposals)"""
    from epievo_amd.host import region_fixed_mask
    opts = opts or {}
    fixed = region_fixed_mask(fp.n_sites, lengths)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=seed)
    o.set_sampler(bool(opts.get("forward_rejection")))
    o.set_proposal_mode(bool(opts.get("reference_proposal_ratio")))
    o.set_sample_root(bool(opts.get("sample_root")))
    o.reset()
    nacc = 0
    for w in range(sweep_base, sweep_base + sweeps):
        for c in range(3):
            for s in range(1, fp.n_sites - 1):
                if s % 3 == c and not fixed[s]:
                    nacc += o.mh_site(s, w)
    return o.paths(), nacc


LAYOUT_A = [3, 61, 64, 65, 63, 3, 341]
LAYOUT_B = [257, 3, 4, 336]
N_SITES = 600
