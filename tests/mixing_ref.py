"""numpy yardstick of the chain mixing diagnostics (include/epievo_mi355x.h, epv_set_mixing): fed the paths of
every sample as FlatPaths, it keeps what the device keeps -- per site the linked sample pairs whose whole history
differs, the sums of the site's jump count x and of its lagged products -- with the histories compared themselves
(init states, jump counts and the bit patterns of the jump times), not through a fingerprint."""
import numpy as np


def history(fp, s):
    """the whole history of site s, walked branch by branch: ((init, (bits of every jump time)), ...)"""
    n, off = fp.n_sites, fp.offsets.astype(np.int64)
    bits = fp.jumps.view(np.uint64)
    return tuple((int(fp.init[b * n + s]), tuple(int(v) for v in bits[off[b * n + s]:off[b * n + s + 1]]))
                 for b in range(fp.n_nodes - 1))


def jump_counts(fp):
    """x of every site: the jumps over all branches, int64 [n]"""
    return fp.counts().reshape(fp.n_nodes - 1, fp.n_sites).sum(axis=0)


def differs(p, q):
    """bool [n]: the sites whose history in p is not the one in q"""
    B, n = p.n_nodes - 1, p.n_sites
    cp, cq = p.counts().reshape(B, n), q.counts().reshape(B, n)
    out = (p.init.reshape(B, n) != q.init.reshape(B, n)).any(axis=0) | (cp != cq).any(axis=0)
    # where all counts agree the jump times pair up one to one: compare their bit patterns
    owner = np.repeat(np.arange(B * n), cp.reshape(-1))
    keep = ~out[owner % n]
    at_p = np.nonzero(keep)[0]
    at_q = q.offsets.astype(np.int64)[owner[keep]] + (at_p - p.offsets.astype(np.int64)[owner[keep]])
    bad = p.jumps.view(np.uint64)[at_p] != q.jumps.view(np.uint64)[at_q]
    out[owner[keep][bad] % n] = True
    return out


class Mixing:
    """the accumulators and the run of one range of sites.  open_run(fp): an opening state; sample(fp, linked): a
    sample, linked to what came before it (the caller applies the rule of who is linked: run_mcmc links all its
    batch samples, an explicit sample is linked when exactly one sweep has passed in an open run); close_run()"""

    def __init__(self, n_sites, max_lag):
        self.K = K = int(max_lag)
        self.samples = self.moved_pairs = 0
        self.pairs = np.zeros(K + 1, np.uint64)
        self.moved = np.zeros(n_sites, np.uint32)
        self.S1, self.S2 = np.zeros(n_sites, np.uint64), np.zeros(n_sites, np.uint64)
        self.C = np.zeros((K, n_sites), np.uint64)
        self.last, self.xs = None, []

    def open_run(self, fp):
        self.last, self.xs = fp, []

    def close_run(self):
        self.last, self.xs = None, []

    def sample(self, fp, linked=True):
        if not linked or self.last is None:
            self.close_run()
        x = jump_counts(fp).astype(np.uint64)
        self.samples += 1
        self.S1 += x
        self.S2 += x * x
        if self.last is not None:
            self.moved_pairs += 1
            self.moved += differs(self.last, fp)
        for k in range(1, min(len(self.xs), self.K) + 1):
            self.pairs[k] += 1
            self.C[k - 1] += x * self.xs[-k]
        self.last = fp
        self.xs = (self.xs + [x])[-self.K:]

    def run_mcmc(self, opening, samples):
        """one run_mcmc call: the state after burn-in, then the paths after every batch sweep"""
        self.open_run(opening)
        for fp in samples:
            self.sample(fp)
        self.close_run()

    def counts(self):
        """what DeviceSampler.mixing(counts=True) returns"""
        return self.samples, self.moved_pairs, self.pairs, self.moved, self.S1, self.S2, self.C


def counts_of_chain(xs, max_lag):
    """the counts of ONE run over the chain xs [samples, sites] of jump counts, the first sample linked to nothing
    -> (samples, moved_pairs, pairs, S1, S2, C)"""
    xs = np.asarray(xs, np.uint64)
    T, K = xs.shape[0], int(max_lag)
    pairs = np.array([0] + [max(0, T - k) for k in range(1, K + 1)], np.uint64)
    C = np.stack([(xs[k:] * xs[:T - k]).sum(axis=0, dtype=np.uint64) if k < T else np.zeros(xs.shape[1], np.uint64)
                  for k in range(1, K + 1)])
    return T, T - 1, pairs, xs.sum(axis=0, dtype=np.uint64), (xs * xs).sum(axis=0, dtype=np.uint64), C


def windows(moved, W, first_site=0, n_global=None):
    """uint64 [ceil(n_global / W)]: moved (of global sites first_site ..) summed over windows of W consecutive global
    sites; zero where it holds no site of a window"""
    n = moved.shape[0]
    n_global = first_site + n if n_global is None else n_global
    nw = (n_global + W - 1) // W
    padded = np.zeros(nw * W, np.uint64)
    padded[first_site:first_site + n] = moved
    return padded.reshape(nw, W).sum(axis=1, dtype=np.uint64)
