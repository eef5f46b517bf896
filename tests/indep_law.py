"""A numpy yardstick for the site-independent two-rate model with soft leaves, shared by test_indep_law.py and
test_indep_leaf_gpu.py (a helper, not a test module).  State 0 leaves at rate r0, state 1 at r1; the root
prior is the chain's stationary law.  A leaf carries a vector q = (q0, q1): the indicator of hard data, (1, 1)
for a missing cell, (1 - r, r) for evidence.  Everything is vectorised over sites: q has shape (N, n, 2).

Route 1 enumerates the joint over all node states; route 2 is Felsenstein pruning and a downward pass."""
import numpy as np


def trans(rates, T):
    """2x2 transition matrix P[from, to] over a branch of length T"""
    r0, r1 = float(rates[0]), float(rates[1])
    s, h = r0 + r1, np.exp(-(r0 + r1) * T)
    return np.array([[(r0 * h + r1) / s, r0 * (1 - h) / s], [r1 * (1 - h) / s, (r0 + r1 * h) / s]])


def prior(rates):
    return np.array([rates[1], rates[0]], np.float64) / (rates[0] + rates[1])


def leaf_q(tree, leaf_state, r=None, mask=None):
    """q (N, n, 2) as the device sets it: leaf_state (N, n) 0/1; r (N-1, n) float32, NaN = none; mask (N-1, n)"""
    N, n = leaf_state.shape
    q = np.ones((N, n, 2))
    for v in range(1, N):
        if tree.subtree_sizes[v] != 1:
            continue
        q[v, :, 1] = leaf_state[v]
        q[v, :, 0] = 1 - leaf_state[v]
        if mask is not None:
            q[v][np.asarray(mask[v - 1]) != 0] = 1.0
        if r is not None:
            rv = np.asarray(r[v - 1], np.float32).astype(np.float64)
            ok = ~np.isnan(rv)
            q[v, ok, 1] = rv[ok]
            q[v, ok, 0] = 1.0 - rv[ok]
    return q


def joint(tree, rates, q):
    """route 1 -> (states (2^N, N), w (2^N, n)): pi(x0) prod_b P_b(x_parent -> x_b) prod_leaf q_leaf(x_leaf)"""
    N = tree.n_nodes
    assert N <= 11, "full enumeration is for small trees"
    x = (np.arange(1 << N)[:, None] >> np.arange(N)) & 1
    w = np.repeat(prior(rates)[x[:, 0]][:, None], q.shape[1], axis=1)
    for v in range(1, N):
        w = w * trans(rates, tree.branches[v])[x[:, tree.parent_ids[v]], x[:, v]][:, None]
        if tree.subtree_sizes[v] == 1:
            w = w * q[v][:, x[:, v]].T
    return x, w


def marginals_enum(tree, rates, q, root=None):
    """route 1: P(state 1) (N, n), with the root state fixed when `root` is 0 or 1; and the likelihood (n,)"""
    x, w = joint(tree, rates, q)
    if root is not None:
        w = w * (x[:, 0] == root)[:, None]
    tot = w.sum(0)
    return np.array([w[x[:, v] == 1].sum(0) for v in range(tree.n_nodes)]) / tot, tot


def marginals_pruning(tree, rates, q):
    """route 2: P(state 1) (N, n) and the likelihood (n,)"""
    N = tree.n_nodes
    a = np.ones_like(q)                       # a[v][:, x] = P(data below v | x_v = x)
    up = np.ones_like(q)                      # up[v][:, x] = P(data below v | x_parent = x)
    for v in range(N - 1, -1, -1):
        if tree.subtree_sizes[v] == 1:
            a[v] = q[v]
        else:
            for c in range(v + 1, v + tree.subtree_sizes[v]):
                if tree.parent_ids[c] == v:
                    a[v] = a[v] * up[c]
        if v:
            up[v] = a[v] @ trans(rates, tree.branches[v]).T
    post = np.zeros_like(q)
    post[0] = prior(rates) * a[0]
    like = post[0].sum(1)
    post[0] /= like[:, None]
    for v in range(1, N):
        P = trans(rates, tree.branches[v])
        u = post[tree.parent_ids[v]] / up[v]                           # (n, x_parent)
        post[v] = (u[:, :, None] * P[None] * a[v][:, None, :]).sum(1)
    return post[:, :, 1], like
