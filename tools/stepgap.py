"""Where a bench.py step spends the time that is in no kernel, from a rocprofv3 --kernel-trace run
(--output-format csv) of

    bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline --no-reference-leg

    python tools/stepgap.py <..._kernel_trace.csv> [--skip 5] [--label NAME]

The launches of one context are strictly ordered on its stream, so the trace is split by stream
(Stream_Id where the trace has one with several values, else Queue_Id; a split under which two
kernels of one group overlap by more than 10 microseconds is refused; smaller crossings of the stamps
count as negative gaps).  The runtime's own fill and copy kernels (hipMemsetAsync, device-to-device
copies) are dispatches of the stream like any other.  Within a stream a step ends with its last
epv_isum_kernel (the statistics reduction that closes run_mcmc) and the next one's chain begins with
its first epv_mh_propose2_kernel; the kernels in between (fill, halo pack and unpack, epv_reset_kernel,
epv_segtab_kernel) belong to the boundary.  Reported per context, as means over the steps after --skip:

  (a) boundary gap: end of the step's last kernel -> start of the next step's first epv_mh_propose2_kernel,
      and how much of it is covered by the boundary's own kernels;
  (b) the mean gap between consecutive kernels of the stream inside a step (first propose2 .. last isum);
  (c) the sum of kernel durations of the stream inside a step, and the step's wall clock
      (first propose2 of a step -> first propose2 of the next);
and the average duration of epv_suffstat_wave_kernel and of the fused colour phase inside those steps.
"""
import argparse
import collections
import csv
import re
import sys

FIRST = "epv_mh_propose2_kernel"
LAST = "epv_isum_kernel"


def short(name):
    name = name.split("(")[0]
    name = (name[5:] if name.startswith("void ") else name).split("<")[0]
    if name.startswith("_Z"):
        m = re.match(r"_Z(\d+)", name)
        name = name[2 + len(m.group(1)):][:int(m.group(1))]
    return name


def load(path):
    rows = list(csv.DictReader(open(path)))
    if not rows:
        sys.exit("%s: no dispatches" % path)
    key = None
    for k in ("Stream_Id", "Queue_Id"):
        if k in rows[0] and len({r[k] for r in rows if short(r["Kernel_Name"]) == FIRST}) > 1:
            key = k
            break
    if key is None:
        sys.exit("%s: neither Stream_Id nor Queue_Id tells the contexts apart" % path)
    streams = collections.defaultdict(list)
    for r in rows:
        streams[r[key]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    out = {}
    for s, ks in streams.items():
        ks.sort()
        if not any(k[2] == FIRST for k in ks):
            continue
        for a, b in zip(ks, ks[1:]):
            # (the stamps of two neighbours of one stream cross by a few hundred nanoseconds on one machine and by
            # up to 4 us on another; two streams taken for one would cross by a kernel's length, tens of us)
            if b[0] + 10000 < a[1]:
                sys.exit("%s %s: %s and %s overlap, this is not one stream" % (key, s, a[2], b[2]))
        out[s] = ks
    return key, out


def steps_of(ks):
    """[(i_first, i_last)]: index of a step's first propose2 and of its last isum"""
    steps, i_first, seen_last = [], None, None
    for i, (_, _, name) in enumerate(ks):
        if name == FIRST:
            if seen_last is not None:       # the previous step is closed by the isum before this launch
                steps.append((i_first, seen_last))
                i_first, seen_last = None, None
            if i_first is None:
                i_first = i
        elif name == LAST and i_first is not None:
            seen_last = i
    if i_first is not None and seen_last is not None:
        steps.append((i_first, seen_last))
    return steps


def mean(v):
    return sum(v) / len(v) if v else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--skip", type=int, default=5, help="leading steps left out (the warm-up)")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    key, streams = load(args.trace)
    print("# %s%s: %d contexts (split by %s), times in microseconds, means over the steps after the first %d"
          % (args.label + " " if args.label else "", args.trace.split("/")[-1], len(streams), key, args.skip))
    tot = collections.defaultdict(list)
    for n_ctx, (s, ks) in enumerate(sorted(streams.items(), key=lambda kv: kv[1][0][0])):
        st = steps_of(ks)[args.skip:]
        gap_a, gap_a_kern, gap_b, sum_c, wall, n_k = [], [], [], [], [], []
        dur = collections.defaultdict(list)
        for q, (i0, i1) in enumerate(st):
            inside = ks[i0:i1 + 1]
            gap_b.append(mean([b[0] - a[1] for a, b in zip(inside, inside[1:])]) / 1e3)
            sum_c.append(sum(k[1] - k[0] for k in inside) / 1e3)
            n_k.append(len(inside))
            for k in inside:
                dur[k[2]].append((k[1] - k[0]) / 1e3)
            if q + 1 < len(st):
                j0 = st[q + 1][0]
                gap_a.append((ks[j0][0] - ks[i1][1]) / 1e3)
                gap_a_kern.append(sum(k[1] - k[0] for k in ks[i1 + 1:j0]) / 1e3)
                wall.append((ks[j0][0] - ks[i0][0]) / 1e3)
        print("context %d (%s %s): %d steps, %.0f kernels per step" % (n_ctx, key, s, len(st), mean(n_k)))
        print("  (a) boundary gap            %9.1f   of which in the boundary's kernels %7.1f, in none %7.1f"
              % (mean(gap_a), mean(gap_a_kern), mean(gap_a) - mean(gap_a_kern)))
        print("  (b) mean gap inside a step  %9.2f   (x %.0f launches = %.1f per step)"
              % (mean(gap_b), mean(n_k) - 1, mean(gap_b) * (mean(n_k) - 1)))
        print("  (c) kernel time inside a step %7.1f   wall clock of a step %9.1f" % (mean(sum_c), mean(wall)))
        for name in sorted(dur):
            v = dur[name]
            print("      %-28s n/step %6.1f  avg %8.2f  min %8.2f  sum/step %9.1f"
                  % (name, len(v) / float(len(st)), mean(v), min(v), sum(v) / len(st)))
        for name, v in (("a", gap_a), ("a_none", [x - y for x, y in zip(gap_a, gap_a_kern)]), ("b", gap_b), ("c", sum_c),
                        ("wall", wall), ("stat", dur.get("epv_suffstat_wave_kernel", [])), ("phase", dur.get(FIRST, []))):
            tot[name] += v
    print("all contexts: (a) %.1f (in no kernel %.1f)  (b) %.2f  (c) %.1f  wall %.1f  epv_suffstat_wave_kernel avg %.2f  "
          "%s avg %.2f" % (mean(tot["a"]), mean(tot["a_none"]), mean(tot["b"]), mean(tot["c"]), mean(tot["wall"]),
                           mean(tot["stat"]), FIRST, mean(tot["phase"])))


if __name__ == "__main__":
    main()
