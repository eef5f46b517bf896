"""numpy yardstick of the posterior branch-event maps (include/epievo_mi355x.h, epv_set_branch_events):
what one sampled history adds to the six planes, from the init state a and the jump count k of every
(branch, site) alone, and the window sums of planes."""
import numpy as np

PLANES = ("end1", "net_gain", "net_loss", "changed", "gains", "losses")


def counts(fp):
    """one sample: uint32 [6, N-1, n]"""
    B, n = fp.n_nodes - 1, fp.n_sites
    a = fp.init.reshape(B, n).astype(np.uint32)
    k = fp.counts().reshape(B, n).astype(np.uint32)
    e = a ^ (k & 1)
    g = (k + (a == 0)) >> 1
    return np.stack([e, (a == 0) & (e == 1), (a == 1) & (e == 0), k >= 1, g, k - g]).astype(np.uint32)


def brute(fp):
    """the same by walking every path: step through its jumps one by one and flip the state"""
    B, n = fp.n_nodes - 1, fp.n_sites
    out = np.zeros((6, B, n), np.uint32)
    off = fp.offsets.astype(np.int64)
    for b in range(B):
        for s in range(n):
            start = state = int(fp.init[b * n + s])
            gains = losses = 0
            for _ in fp.jumps[off[b * n + s]:off[b * n + s + 1]]:
                if state == 0:
                    gains += 1
                else:
                    losses += 1
                state = 1 - state
            out[:, b, s] = [state, start == 0 and state == 1, start == 1 and state == 0, gains + losses > 0,
                            gains, losses]
    return out


def windows(planes, W, first_site=0, n_global=None):
    """uint64 [6, N-1, ceil(n_global / W)]: planes (of global sites first_site ..) summed over windows of W
    consecutive global sites; zero where the planes hold no site of a window"""
    n = planes.shape[2]
    n_global = first_site + n if n_global is None else n_global
    nw = (n_global + W - 1) // W
    if W >= n_global:
        return planes.sum(axis=2, dtype=np.uint64)[:, :, None]
    padded = np.zeros(planes.shape[:2] + (nw * W,), np.uint64)       # zero outside the planes' sites
    padded[:, :, first_site:first_site + n] = planes
    return padded.reshape(planes.shape[:2] + (nw, W)).sum(axis=3, dtype=np.uint64)


def start1(planes):
    """the state at the parent end of every branch: end1 - net_gain + net_loss (as signed numbers)"""
    p = planes.astype(np.int64)
    return p[0] - p[1] + p[2]


def parse_changes(text):
    """the -c file of epievo_est_histories -> (samples, W, node names, branch-length strings,
    first sites [windows], uint64 sums [6, nodes, windows])"""
    lines = text.splitlines()
    head = lines[0].split("\t")
    assert head[0] == "#samples" and head[2] == "window", head
    names, blens, blocks = [], [], []
    for ln in lines[1:]:
        if ln.startswith("NODE:"):
            name, blen = ln[5:].split("\t")
            names.append(name)
            blens.append(blen)
            blocks.append([])
        else:
            blocks[-1].append([int(v) for v in ln.split("\t")])
    arr = np.array(blocks, np.uint64)                 # [nodes, windows, 7]
    return int(head[1]), int(head[3]), names, blens, arr[0, :, 0], np.moveaxis(arr[:, :, 1:], 2, 0)
