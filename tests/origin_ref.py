"""numpy yardstick of the lineage origin maps (include/epievo_mi355x.h, epv_set_lineage_origins): the row
table, the fixed-point scale, what one sampled history adds to origin [R, n] and age [L, n], window sums,
and the same sample by a plain per-site walk."""
import math

import numpy as np

MAX_SAMPLES = 2 ** 21


def tables(tree):
    """-> dict(leaves [L], first [L + 1], rows uint32 [R, 2] (leaf node, branch node or 0), H, k, fixT int64 [N])"""
    parent, sub, T = np.asarray(tree.parent_ids), np.asarray(tree.subtree_sizes), np.asarray(tree.branches, np.float64)
    leaves = [v for v in range(1, tree.n_nodes) if sub[v] == 1]
    first, rows, H = [], [], 0.0
    for leaf in leaves:
        first.append(len(rows))
        h, v = 0.0, leaf
        while v != 0:
            rows.append((leaf, v))
            h += float(T[v])                       # fp64, from the leaf upward
            v = int(parent[v])
        rows.append((leaf, 0))
        if not h <= H:
            H = h
    first.append(len(rows))
    k = 0
    if H > 0.0 and math.isfinite(H):
        k = max(-1000, min(1000, 40 - math.frexp(H)[1]))
    fixT = np.rint(np.ldexp(T, k)).astype(np.int64)
    fixT[0] = 0
    return dict(leaves=leaves, first=first, rows=np.array(rows, np.uint32).reshape(-1, 2), H=H, k=k, fixT=fixT)


def sample(fp, tree, tab=None):
    """one sample: (origin uint32 [R, n], age uint64 [L, n])"""
    tab = tab or tables(tree)
    B, n = fp.n_nodes - 1, fp.n_sites
    cnt = fp.counts().reshape(B, n)
    end = fp.offsets[1:].astype(np.int64).reshape(B, n)        # one past the last jump of every path
    T, rows, fixT, scale = np.asarray(tree.branches, np.float64), tab["rows"], tab["fixT"], 2.0 ** tab["k"]
    origin = np.zeros((len(rows), n), np.uint32)
    age = np.zeros((len(tab["leaves"]), n), np.int64)
    for li in range(len(tab["leaves"])):
        found, held = np.zeros(n, bool), 0
        for r in range(tab["first"][li], tab["first"][li + 1] - 1):
            v = int(rows[r, 1])
            hit = ~found & (cnt[v - 1] >= 1)
            origin[r, hit] = 1
            t_last = fp.jumps[end[v - 1, hit] - 1]
            age[li, hit] = held + np.rint((T[v] - t_last) * scale).astype(np.int64)
            found |= hit
            held += int(fixT[v])
        origin[tab["first"][li + 1] - 1, ~found] = 1
        age[li, ~found] = held
    return origin, age.astype(np.uint64)


def brute(fp, tree):
    """the same by walking, site by site, up every leaf's lineage through the parent array"""
    parent, sub, T = tree.parent_ids, tree.subtree_sizes, tree.branches
    tab = tables(tree)
    B, n = fp.n_nodes - 1, fp.n_sites
    off = fp.offsets.astype(np.int64)
    row_of = {(int(a), int(b)): r for r, (a, b) in enumerate(tab["rows"])}
    leaves = [v for v in range(1, tree.n_nodes) if sub[v] == 1]
    origin = np.zeros((len(row_of), n), np.uint32)
    age = np.zeros((len(leaves), n), np.uint64)
    for li, leaf in enumerate(leaves):
        for s in range(n):
            v, held = leaf, 0
            while v != 0:
                e = (v - 1) * n + s
                if off[e + 1] > off[e]:
                    last = float(fp.jumps[off[e + 1] - 1])
                    held += int(np.rint((float(T[v]) - last) * 2.0 ** tab["k"]))
                    break
                held += int(tab["fixT"][v])
                v = int(parent[v])
            origin[row_of[(leaf, v)], s] += 1
            age[li, s] = held
    return origin, age


def windows(cells, W, first_site=0, n_global=None):
    """uint64 [rows, ceil(n_global / W)]: cells [rows, n] (of global sites first_site ..) summed over windows of
    W consecutive global sites; zero where the cells hold no site of a window"""
    n = cells.shape[1]
    n_global = first_site + n if n_global is None else n_global
    nw = (n_global + W - 1) // W
    if W >= n_global:
        return cells.sum(axis=1, dtype=np.uint64)[:, None]
    padded = np.zeros((cells.shape[0], nw * W), np.uint64)
    padded[:, first_site:first_site + n] = cells
    return padded.reshape(cells.shape[0], nw, W).sum(axis=2, dtype=np.uint64)


def check_invariants(tree, origin, age, ns, changed=None, tab=None):
    """what must hold per cell of any result of ns samples; changed: the branch events' plane 3 [N-1, n]"""
    tab = tab or tables(tree)
    o = origin.astype(np.int64)
    for li in range(len(tab["leaves"])):
        r0, r1 = tab["first"][li], tab["first"][li + 1]
        assert (o[r0:r1].sum(axis=0) == ns).all()                       # a leaf's rows sum to the sample count
        full = ns * int(sum(int(tab["fixT"][v]) for v in tab["rows"][r0:r1 - 1, 1]))
        a = age[li].astype(np.int64)
        assert (a <= full).all() and np.array_equal(a == full, o[r1 - 1] == ns)
        if changed is not None:
            assert np.array_equal(o[r0], changed[tab["leaves"][li] - 1].astype(np.int64))   # the leaf-branch row
