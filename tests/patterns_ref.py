"""numpy yardstick of the change patterns (include/epievo_mi355x.h, epv_set_change_patterns): what one sampled
history adds to the R = 12 + 2 (N-1) + I rows, from the init state a and the jump count k of every (branch, site)
and the tree alone; a brute-force walk that shares no logic with it; the window sums; the parser of the -P file."""
import numpy as np

FIXED = ("jumps_1", "jumps_2", "jumps_3", "jumps_4", "jumps_5", "jumps_6", "jumps_7plus", "one_branch",
         "parallel_gain", "parallel_loss", "gain_and_loss", "reverted_only")
ONE_BRANCH, PAR_GAIN, PAR_LOSS, GAIN_AND_LOSS, REVERTED = 7, 8, 9, 10, 11


def clade_nodes(tree):
    """the internal non-root nodes in pre-order"""
    return [v for v in range(1, tree.n_nodes) if tree.subtree_sizes[v] > 1]


def n_rows(tree):
    return 12 + 2 * (tree.n_nodes - 1) + len(clade_nodes(tree))


def row_names(tree):
    nodes = range(1, tree.n_nodes)
    return (list(FIXED) + ["sole_gain:" + tree.node_names[v] for v in nodes] +
            ["sole_loss:" + tree.node_names[v] for v in nodes] +
            ["clade_changed:" + tree.node_names[v] for v in clade_nodes(tree)])


def counts(fp, tree):
    """one sample: uint32 [R, n]"""
    B, n = fp.n_nodes - 1, fp.n_sites
    a = fp.init.reshape(B, n).astype(np.int64)
    k = fp.counts().reshape(B, n).astype(np.int64)
    odd = k & 1
    c, K = (k >= 1).sum(axis=0), k.sum(axis=0)
    gain, loss = (a == 0) & (odd == 1), (a == 1) & (odd == 1)
    ng, nl = gain.sum(axis=0), loss.sum(axis=0)
    rows = [K == h for h in range(1, 7)] + [K >= 7, c == 1, ng >= 2, nl >= 2, (ng >= 1) & (nl >= 1),
                                            (c >= 1) & (ng == 0) & (nl == 0)]
    rows += [(c == 1) & gain[b] for b in range(B)] + [(c == 1) & loss[b] for b in range(B)]
    for v in clade_nodes(tree):                      # branches v .. v + subtree - 2 belong to nodes v+1 .. v+subtree-1
        rows.append(k[v:v + int(tree.subtree_sizes[v]) - 1].sum(axis=0) >= 1)
    return np.stack(rows).astype(np.uint32)


def brute(fp, tree):
    """the same by walking every path jump by jump; the nodes below a node are found by following parent_ids
    upward from every node, not by pre-order ranges"""
    N, n = fp.n_nodes, fp.n_sites
    B = N - 1
    parent = [int(p) for p in tree.parent_ids]
    children = {v: 0 for v in range(N)}
    for v in range(1, N):
        children[parent[v]] += 1
    clades = [v for v in range(1, N) if children[v] > 0]
    below = {v: [] for v in clades}                  # the nodes strictly below v
    for u in range(1, N):
        w = parent[u]
        while w != 0:
            below[w].append(u)
            w = parent[w]
    out = np.zeros((12 + 2 * B + len(clades), n), np.uint32)
    off = fp.offsets.astype(np.int64)
    for s in range(n):
        jumps, net = [0] * N, [0] * N                # per node: jumps on its branch, end state - start state
        for v in range(1, N):
            i = (v - 1) * n + s
            start = state = int(fp.init[i])
            for _ in fp.jumps[off[i]:off[i + 1]]:
                state = 1 - state
                jumps[v] += 1
            net[v] = state - start
        total = sum(jumps)
        changed = [v for v in range(1, N) if jumps[v] > 0]
        gains, losses = [v for v in changed if net[v] > 0], [v for v in changed if net[v] < 0]
        if total:
            out[min(total, 7) - 1, s] = 1
        if len(changed) == 1:
            out[ONE_BRANCH, s] = 1
            for v in gains:
                out[12 + v - 1, s] = 1
            for v in losses:
                out[12 + B + v - 1, s] = 1
        out[PAR_GAIN, s] = len(gains) >= 2
        out[PAR_LOSS, s] = len(losses) >= 2
        out[GAIN_AND_LOSS, s] = bool(gains) and bool(losses)
        out[REVERTED, s] = bool(changed) and not gains and not losses
        for j, v in enumerate(clades):
            out[12 + 2 * B + j, s] = any(jumps[u] for u in below[v])
    return out


def windows(rows, W, first_site=0, n_global=None):
    """uint64 [R, ceil(n_global / W)]: rows (of global sites first_site ..) summed over windows of W consecutive
    global sites; zero where the rows hold no site of a window"""
    n = rows.shape[1]
    n_global = first_site + n if n_global is None else n_global
    nw = (n_global + W - 1) // W
    if W >= n_global:
        return rows.sum(axis=1, dtype=np.uint64)[:, None]
    padded = np.zeros((rows.shape[0], nw * W), np.uint64)            # zero outside the rows' sites
    padded[:, first_site:first_site + n] = rows
    return padded.reshape(rows.shape[0], nw, W).sum(axis=2, dtype=np.uint64)


def parse_patterns(text):
    """the -P file of epievo_est_histories -> (samples, W, sites, row names, first sites [windows],
    uint64 sums [R, windows])"""
    lines = text.splitlines()
    head = lines[0].split("\t")
    assert head[0] == "#samples" and head[2] == "window" and head[4] == "sites", head
    names = lines[1].split("\t")
    assert names[0] == "#rows", names[0]
    arr = np.array([[int(v) for v in ln.split("\t")] for ln in lines[2:]], np.uint64).reshape(-1, len(names))
    return int(head[1]), int(head[3]), int(head[5]), names[1:], arr[:, 0], np.ascontiguousarray(arr[:, 1:].T)
