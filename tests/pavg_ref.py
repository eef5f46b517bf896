"""numpy restatement of the reference's average_paths (src/prog/average_paths.cpp:31-63) with the
per-branch fix (node b's own path for every point; the reference reads node 1's at points >= 1),
the checker of the average_paths CLI and of the device counts."""
import numpy as np


def grid(tot_time, n_points):
    """t_0 = 0, t_1 = bin, t_{i+1} = t_i + bin: repeated fp64 addition, as the reference does it"""
    b = tot_time / (n_points - 1)
    t, cur = [0.0], b
    for _ in range(1, n_points):
        t.append(cur)
        cur += b
    return np.array(t)


def counts(fp, tot_times, n_points):
    """one sample: uint32 [N-1, n, P], the path's state at every grid point (init at point 0,
    state_at_time = init XOR parity of lower_bound(jumps, t_i) at points >= 1)"""
    B, n = fp.n_nodes - 1, fp.n_sites
    init = fp.init.reshape(B, n).astype(np.uint32)
    out = np.repeat(init[:, :, None], n_points, axis=2)
    off = fp.offsets.astype(np.int64)
    for b in range(B):
        t = grid(float(tot_times[b + 1]), n_points)[1:]
        for s in np.nonzero(off[b * n + 1:(b + 1) * n + 1] > off[b * n:(b + 1) * n])[0]:
            e = b * n + s
            idx = np.searchsorted(fp.jumps[off[e]:off[e + 1]], t, side="left")
            out[b, s, 1:] = init[b, s] ^ (idx & 1)
    return out


def format_average(node_names, branch_len, cnt, n_samples):
    """write_output (average_paths.cpp:49-63): C++ default ostream formatting = %g"""
    lines = ["NODE:%s" % node_names[0]]
    avg = cnt / float(n_samples)
    for b in range(1, len(node_names)):
        lines.append("NODE:%s\t%s" % (node_names[b], "%g" % branch_len[b]))
        lines.extend("\t".join("%g" % v for v in row) for row in avg[b - 1])
    return "\n".join(lines) + "\n"
