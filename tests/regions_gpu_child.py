"""One GPU case of tests/test_regions_gpu.py in a process of its own (a context reads its EPV_* knobs when it is
created): python regions_gpu_child.py '<json spec>'.  Prints one line "ok <json>"."""
import json
import os
import sys

import numpy as np

_TESTS = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_TESTS))
sys.path.insert(0, _TESTS)

import orc                                          # noqa: E402
import regions_ref as rr                            # noqa: E402
from common import ref_test_model                   # noqa: E402
from epievo_amd import host                         # noqa: E402
from epievo_amd.sampler import DeviceSampler       # noqa: E402
from test_kernel_matrix import make_tree            # noqa: E402

SEED, BURN_IN, BATCH, BASE = 19, 2, 3, 4


def inputs(spec):
    model, tree = ref_test_model(), make_tree(spec.get("tree", "tree"))
    fp = host.simulate(model, tree, spec.get("n", rr.N_SITES), 6)
    return model, tree, fp, int(max(16, 2 * fp.counts().max() + 8))


def leaf_mask(tree, n):
    """every seventh cell of every leaf branch, staggered by branch: cells of fixed and of free sites, all three colours"""
    B = tree.n_nodes - 1
    mask = np.zeros((B, n), np.uint8)
    for node in range(1, tree.n_nodes):
        if tree.subtree_sizes[node] == 1:
            mask[node - 1, node % 7::7] = 1
    return mask


def context(spec, model, tree, fp, cap, mask=None, sites=None, update=None):
    """a context with the row's options on the whole genome, or on the columns sites = (lo, hi) with update = (first,
    last) as its update range"""
    d = DeviceSampler(0)
    d.set_tree(tree)
    d.set_model(model)
    if sites:
        d.upload_paths(fp.slice_sites(*sites), cap, sites[0], fp.n_sites)
        d.set_update_range(*update)
    else:
        d.upload_paths(fp, cap)
    d.set_options(**spec.get("opts", {}))
    if spec.get("direct"):
        d.set_direct_sampler(True, fused=bool(spec.get("direct_fused")))
    if spec.get("leaf_fast"):
        d.set_leaf_fast(True)
    if spec.get("leaf"):
        m = leaf_mask(tree, fp.n_sites)
        d.set_unobserved(m[:, sites[0]:sites[1]] if sites else m)
    if mask is not None:
        d.set_fixed_sites(mask)
    d.reset()
    return d


def check_plan(d, expect):
    plan = d.phase_plan()
    bad = dict((k, (v, plan[k])) for k, v in expect.items() if plan[k] != v)
    assert not bad, "plan differs (expected, got): %r; plan %r" % (bad, plan)
    return plan


def device_regions_ref(spec, model, tree, fp, cap, lengths):
    """the reference of the rows the oracle has no sampler for (the direct sampler): every region run alone ON THE
    DEVICE, a context of its own over the region's columns and the one context column at each end where the genome
    goes on (as regions_ref cuts them), the inner sites as its update range -- the mechanism of the sharded runs,
    which never updates or counts a site outside the range -> (counts, accepted, paths by region, tri by region)"""
    n = fp.n_sites
    counts, nacc, paths, tri = 0, 0, [], []
    for a, m in zip(rr.region_starts(lengths), lengths):
        lo, hi = (a - 1 if a > 0 else a), (a + m + 1 if a + m < n else a + m)
        off = a - lo
        d = context(spec, model, tree, fp, cap, sites=(lo, hi), update=(off + 1, off + m - 2))
        c, k = d.run_mcmc_counts(BURN_IN, BATCH, SEED, BASE)
        counts, nacc = counts + c, nacc + k
        paths.append(d.paths().slice_sites(off, off + m))
        tri.append(d.tri_llh()[off:off + m])
        d.close()
    return counts, nacc, paths, tri


def run_row(spec):
    """one kernel family under regions: run_mcmc_counts(2, 3) against the per-region reference, bit for bit"""
    from epievo_amd.parallel import concat_sites
    model, tree, fp, cap = inputs(spec)
    lengths = spec["layout"]
    mask = host.region_fixed_mask(fp.n_sites, lengths)
    d = context(spec, model, tree, fp, cap, mask)
    plan = check_plan(d, spec["expect"])
    assert d.fixed_sites() == int(mask[1:-1].sum())
    before = d.paths()
    counts, nacc = d.run_mcmc_counts(BURN_IN, BATCH, SEED, BASE)
    after, tri = d.paths(), d.tri_llh()
    assert d.phase_plan() == plan
    if spec.get("direct"):
        want_counts, want_nacc, rp, rt = device_regions_ref(spec, model, tree, fp, cap, lengths)
        want_paths, want_tri = concat_sites(rp), np.concatenate(rt)
    else:
        ref = rr.RegionsRef(tree, model, fp, lengths, cap, SEED, spec.get("opts"),
                            leaf_mask(tree, fp.n_sites) if spec.get("leaf") else None)
        want_counts, want_nacc = ref.run_mcmc_counts(BURN_IN, BATCH, BASE)
        want_paths, want_tri = ref.paths(), ref.tri_llh()
    starts = rr.region_starts(lengths)
    differ = [k for k, (a, m) in enumerate(zip(starts, lengths))
              if not orc.paths_equal(after.slice_sites(a, a + m), want_paths.slice_sites(a, a + m))]
    assert not differ, "the paths of regions %r differ (accepted %d, reference %d)" % (differ, nacc, want_nacc)
    assert nacc == want_nacc, (nacc, want_nacc)
    assert np.array_equal(counts, want_counts), np.argwhere(counts != want_counts)[:8]
    assert orc.paths_equal(after, want_paths)
    free = mask == 0
    assert np.array_equal(tri[free].view(np.uint64), want_tri[free].view(np.uint64))
    # a fixed site's path is what it was, to the bit
    B, n = tree.n_nodes - 1, fp.n_sites
    for s in np.nonzero(mask)[0]:
        a, b = before.slice_sites(int(s), int(s) + 1), after.slice_sites(int(s), int(s) + 1)
        assert orc.paths_equal(a, b), int(s)
    assert nacc > 0 and not orc.paths_equal(before, after)
    # the doubles of run_mcmc's other entry point are these integers
    d2 = context(spec, model, tree, fp, cap, mask)
    J2, D2, n2 = d2.run_mcmc(BURN_IN, BATCH, SEED, BASE)
    Jc, Dc = d.counts_to_stats(counts, BATCH, True)
    assert n2 == nacc and np.array_equal(J2, Jc) and np.array_equal(D2, Dc)
    # ... and epv_get_sufficient_statistics counts the resident paths like the last batch sweep
    Js, Ds = d2.suffstats()
    Jl, Dl = d.counts_to_stats(counts[-1:], 1, False)
    assert np.array_equal(Js, Jl) and np.array_equal(Ds, Dl)
    d.close()
    d2.close()
    return dict(plan=plan, nacc=int(nacc))


def run_default(spec):
    """no mask, and an all-zero mask: the whole-genome oracle's run, and the same counters and timed launches"""
    model, tree, fp, cap = inputs(spec)
    o = orc.Oracle(tree, model, fp, "B", cap=cap, seed=SEED)
    o.reset()
    Jo, Do, no, _ = o.run_mcmc(BURN_IN, BATCH, sweep_base=BASE)
    seen = []
    for mask in (None, np.zeros(fp.n_sites, np.uint8), "cleared"):
        cleared = isinstance(mask, str)     # a mask that was set and taken away again
        d = context(spec, model, tree, fp, cap, host.region_fixed_mask(fp.n_sites, rr.LAYOUT_A) if cleared else mask)
        if cleared:
            d.set_fixed_sites(None)
        assert d.fixed_sites() == 0
        d.set_timing(1)
        J, D, nacc = d.run_mcmc(BURN_IN, BATCH, SEED, BASE)
        assert nacc == no and np.array_equal(J, Jo) and np.array_equal(D, Do)
        assert orc.paths_equal(d.paths(), o.paths())
        assert np.array_equal(d.tri_llh().view(np.uint64), o.tri_llh().view(np.uint64))
        seen.append((d.counters(), d.kernel_time_ms()[1], d.phase_plan()))
        d.close()
    assert seen[0] == seen[1] == seen[2], seen
    assert seen[0][1] == 3 * (BURN_IN + BATCH)
    return dict(launches=seen[0][1])


def _swap_inner(fp, other, a, m):
    from epievo_amd.parallel import concat_sites
    return concat_sites([fp.slice_sites(0, a + 1), other.slice_sites(a + 1, a + m - 1), fp.slice_sites(a + m - 1, fp.n_sites)])


def run_decoupling(spec):
    """other data inside one region (its inner columns, leaf states with them): every other region's paths and
    integer statistics are what they were, and the totals move by that region's statistics alone"""
    import ctypes as C
    model, tree, fp, cap = inputs(spec)
    lengths, k = spec["layout"], spec["region"]
    a, m = rr.region_starts(lengths)[k], lengths[k]
    other = host.simulate(model, tree, fp.n_sites, 77)
    fq = _swap_inner(fp, other, a, m)
    cap = int(max(cap, 2 * fq.counts().max() + 8))
    leaf = np.asarray(tree.subtree_sizes)[1:] == 1
    ends = lambda p: (p.init ^ (p.counts() & 1).astype(np.uint8)).reshape(tree.n_nodes - 1, -1)[leaf]
    assert (ends(fp) != ends(fq))[:, a + 1:a + m - 1].any() and np.array_equal(ends(fp)[:, :a + 1], ends(fq)[:, :a + 1])
    mask = host.region_fixed_mask(fp.n_sites, lengths)
    runs = []
    for data in (fp, fq):
        d = context(spec, model, tree, data, cap, mask)
        counts, nacc = d.run_mcmc_counts(BURN_IN, BATCH, SEED, BASE)
        p = d.paths()
        o = orc.Oracle(tree, model, p, "B", cap=cap)     # (the integer statistics of the sampled paths, region by region)
        rows = np.zeros((len(lengths), tree.n_nodes - 1, 16), np.int64)
        for r, (ra, rm) in enumerate(zip(rr.region_starts(lengths), lengths)):
            one = np.zeros((1, tree.n_nodes - 1, 16), np.int64)
            o.L.orc_suffstats_rows(o.h, 0, fp.n_sites, 1, ra + 1, ra + rm - 2, orc._p(one, C.c_int64))
            rows[r] = one[0]
        assert np.array_equal(rows.sum(axis=0).reshape(-1), counts[-1])
        runs.append((p, rows, counts))
        d.close()
    (p0, rows0, c0), (p1, rows1, c1) = runs
    for r, (ra, rm) in enumerate(zip(rr.region_starts(lengths), lengths)):
        same = orc.paths_equal(p0.slice_sites(ra, ra + rm), p1.slice_sites(ra, ra + rm)) and np.array_equal(rows0[r], rows1[r])
        assert same == (r != k), (r, same)
    assert np.array_equal(c1[-1] - c0[-1], (rows1[k] - rows0[k]).reshape(-1))
    return dict(region=k)


def run_lifetime(spec):
    """the mask outlives a capacity overflow and the regrow, scale_jump_times and a second reset"""
    model, tree, fp, _ = inputs(spec)
    lengths = spec["layout"]
    mask = host.region_fixed_mask(fp.n_sites, lengths)
    n_fixed = int(mask[1:-1].sum())
    cap = int(fp.counts().max())          # a capacity that overflows
    d = context(spec, model, tree, fp, cap, mask)
    d.auto_grow = True
    ref = rr.RegionsRef(tree, model, fp, lengths, cap, SEED)
    counts, nacc = d.run_mcmc_counts(BURN_IN, BATCH, SEED, BASE)
    want, want_nacc = ref.run_mcmc_counts(BURN_IN, BATCH, BASE)
    # (the overflows of non-fixed sites are the reference's; a fixed site's unused proposal may add to the device's)
    assert ref.overflow() > 0 and d.counters()["overflow"] >= ref.overflow()
    assert d.capacity_events and d.capacity() == 2 * cap and d.fixed_sites() == n_fixed
    assert nacc == want_nacc and np.array_equal(counts, want) and orc.paths_equal(d.paths(), ref.paths())

    def again(base, tree_now):
        p = d.paths()
        r = rr.RegionsRef(tree_now, model, p, lengths, d.capacity(), SEED)
        d.reset()
        c, k = d.run_mcmc_counts(1, 2, SEED, base)
        wc, wk = r.run_mcmc_counts(1, 2, base)
        assert k == wk and np.array_equal(c, wc) and orc.paths_equal(d.paths(), r.paths())
        assert d.fixed_sites() == n_fixed
        for s in np.nonzero(mask)[0]:
            assert orc.paths_equal(p.slice_sites(int(s), int(s) + 1), d.paths().slice_sites(int(s), int(s) + 1))

    again(20, tree)                       # the repeat at the grown capacity, after a second reset
    nb = tree.branches * 1.1
    d.scale_jump_times(nb)
    d.set_model(model)
    again(30, host.Tree(tree.subtree_sizes, tree.parent_ids, nb))
    # new paths clear it, as they clear the mask of unobserved cells
    d.upload_paths(fp, 2 * cap)
    assert d.fixed_sites() == 0
    d.close()
    return dict(capacity=2 * cap)


def run_group(spec):
    """LocalGroup(shards = 3) with regions: the single context's integers, accept count and paths"""
    from epievo_amd.parallel import LocalGroup
    model, tree, fp, cap = inputs(spec)
    lengths = spec["layout"]
    mask = host.region_fixed_mask(fp.n_sites, lengths)
    d = context(spec, model, tree, fp, cap, mask)
    g = LocalGroup(0, 3)
    g.set_tree(tree)
    g.set_model(model)
    g.upload_paths(fp, cap)
    assert len(g.subs) == 3 and g.b[:2] == spec["cuts"], g.b
    g.set_regions(lengths)
    g.reset()
    assert g.fixed_sites() == d.fixed_sites() == int(mask[1:-1].sum())
    cd, nd = d.run_mcmc_counts(BURN_IN, BATCH, SEED, BASE)
    cg, ng = g.run_mcmc_counts(BURN_IN, BATCH, SEED, BASE)
    assert nd == ng and np.array_equal(cd, cg) and orc.paths_equal(d.paths(), g.paths())
    # new paths: the group applies its regions again
    g.upload_paths(fp, cap)
    g.reset()
    assert g.fixed_sites() == int(mask[1:-1].sum())
    cg2, ng2 = g.run_mcmc_counts(BURN_IN, BATCH, SEED, BASE)
    assert ng2 == nd and np.array_equal(cg2, cd)
    g.close()
    d.close()
    return dict(nacc=int(nd))


def run_cpp(spec):
    """the C++ driver over the contexts EPV_DEVICES names: the single context's J, D, acceptance rate and paths"""
    from epievo_amd.driver import CppSampler
    model, tree, fp, cap = inputs(spec)
    lengths = spec["layout"]
    mask = host.region_fixed_mask(fp.n_sites, lengths)
    d = context(spec, model, tree, fp, cap, mask)
    counts, nacc = d.run_mcmc_counts(BURN_IN, BATCH, SEED, 0)
    J, D = d.counts_to_stats(counts, BATCH, True)
    devices = [int(x) for x in os.environ["EPV_DEVICES"].split(",")]
    s = CppSampler(BURN_IN, BATCH, devices=devices, capacity=cap)
    s.set_regions(lengths)                 # before the paths: applied by reset
    s.reset(model, tree, fp)
    lay = s.layout()
    assert lay["slots_here"] == len(devices) and lay["parts_here"] >= len(devices), lay
    Jc, Dc, acc = s.run_mcmc(SEED, 0)
    assert np.array_equal(Jc, J) and np.array_equal(Dc, D)
    assert acc == nacc / float(BATCH * (fp.n_sites - 2 - int(mask[1:-1].sum())))
    assert orc.paths_equal(s.paths(), d.paths())
    # taken away and set again while paths are resident
    s.set_regions(None)
    s.set_regions(lengths)
    s.reset(model, tree, fp)
    Jc2, Dc2, acc2 = s.run_mcmc(SEED, 0)
    assert np.array_equal(Jc2, J) and np.array_equal(Dc2, D) and acc2 == acc
    try:
        s.enable_window_stats(50)
        raise AssertionError("the window statistics went on over regions")
    except Exception as e:
        assert "fixed sites are held (epv_set_fixed_sites) and the window statistics would count across them" in str(e), e
    s.close()
    d.close()
    return dict(layout=lay["text"])


def run_cli(spec):
    """epievo_est_histories -G: the Python result; -G with -r and a regions file of the wrong length are refused"""
    import subprocess
    from epievo_amd import _build
    from epievo_amd.sampler import SingleSiteSampler
    from epievo_amd.workloads import TEST_PARAM_TEXT, TREE_NWK_TEXT
    tmp, lengths = spec["tmp"], spec["layout"]
    write = lambda name, text: open(os.path.join(tmp, name), "w").write(text)
    write("t.nwk", TREE_NWK_TEXT)
    write("p.param", TEST_PARAM_TEXT)
    model, tree = ref_test_model(), host.Tree.read(os.path.join(tmp, "t.nwk"))
    fp = host.simulate(model, tree, rr.N_SITES, 12)
    host.write_paths(os.path.join(tmp, "in.paths"), tree.node_names, tree.branches, fp)
    write("genome.sizes", "# name n_sites\n" + "".join("chr%d\t%d\n" % (k + 1, m) for k, m in enumerate(lengths)))
    write("short.sizes", "".join("chr%d %d\n" % (k + 1, m) for k, m in enumerate(lengths[:-1])))

    def run(program, out, *extra):
        cmd = [os.path.join(_build.BIN_DIR, program), "-L", str(BURN_IN), "-B", str(BATCH), "-s", "17", "-o",
               os.path.join(tmp, out)] + list(extra) + [os.path.join(tmp, x) for x in ("p.param", "t.nwk", "in.paths")]
        return subprocess.run(cmd, capture_output=True, text=True, timeout=300)

    r = run("epievo_est_histories", "out.paths", "-G", os.path.join(tmp, "genome.sizes"))
    assert r.returncode == 0, r.stderr[-2000:]
    s = SingleSiteSampler(BURN_IN, BATCH)
    assert host.read_regions(os.path.join(tmp, "genome.sizes"), fp.n_sites) == lengths
    s.set_regions(lengths)
    s.reset(model, tree, fp)
    s.run_mcmc(17, 0)
    got, _, _ = host.read_paths(os.path.join(tmp, "out.paths"))
    assert orc.paths_equal(got, s.paths())
    plain = run("epievo_est_histories", "plain.paths")
    assert plain.returncode == 0 and not orc.paths_equal(host.read_paths(os.path.join(tmp, "plain.paths"))[0], got)
    r = run("epievo_est_histories", "no.paths", "-G", os.path.join(tmp, "genome.sizes"), "-r", os.path.join(tmp, "r.txt"))
    assert r.returncode != 0 and "fixed sites are held (epv_set_fixed_sites) and the window statistics would count " \
        "across them" in r.stderr, r.stderr[-2000:]
    r = run("epievo_est_histories", "no.paths", "-G", os.path.join(tmp, "short.sizes"))
    assert r.returncode != 0 and "short.sizes, line %d: the regions hold %d sites in all, the paths hold %d" % (
        len(lengths) - 1, sum(lengths[:-1]), fp.n_sites) in r.stderr, r.stderr[-2000:]
    # the EM driver takes the file too, and its runs differ from the ones without
    outs = []
    for tag, extra in (("em-regions", ["-G", os.path.join(tmp, "genome.sizes")]), ("em-plain", [])):
        r = run("epievo_est_params_histories", tag + ".paths", "-i", "2", "-p", os.path.join(tmp, tag + ".param"), *extra)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(host.read_paths(os.path.join(tmp, tag + ".paths"))[0])
    mask = host.region_fixed_mask(fp.n_sites, lengths)
    for site in np.nonzero(mask)[0][1:-1]:
        held = outs[0].slice_sites(int(site), int(site) + 1)
        assert np.array_equal(held.init, fp.slice_sites(int(site), int(site) + 1).init) and \
            np.array_equal(held.counts(), fp.slice_sites(int(site), int(site) + 1).counts())
    assert not orc.paths_equal(outs[0], outs[1])
    return dict(regions=len(lengths))


REFUSING = [("window_stats", (50,), "the window statistics"), ("epoch_stats", (4,), "the epoch statistics"),
            ("domain_stats", (8,), "the domain statistics"), ("domain_turnover", (8,), "the domain turnover"),
            ("change_tracts", (8,), "the change tracts"), ("spatial_correlation", (4, 8), "the spatial correlations"),
            ("domain_maps", ([2, 5], 1, 8), "the domain maps")]


def run_refusing(spec):
    """the seven layers that count across neighbouring sites and the fixed sites refuse each other, either order"""
    from epievo_amd.sampler import EpvError
    model, tree, fp, cap = inputs(spec)
    mask = host.region_fixed_mask(fp.n_sites, spec["layout"])
    d = context(spec, model, tree, fp, cap)
    for stem, args, name in REFUSING:
        off = ([],) if stem == "domain_maps" else (0,) * (2 if stem == "spatial_correlation" else 1)
        d.set_fixed_sites(mask)
        try:
            getattr(d, "enable_" + stem)(*args)
            raise AssertionError("enable_%s went through over fixed sites" % stem)
        except EpvError as e:
            assert str(e) == ("epv error 4: epv_set_%s: fixed sites are held (epv_set_fixed_sites) and %s would count "
                              "across them: clear the fixed sites first" % (stem, name)), str(e)
        getattr(d, "enable_" + stem)(*off)            # switching it off is no offence
        d.set_fixed_sites(None)
        getattr(d, "enable_" + stem)(*args)
        try:
            d.set_fixed_sites(mask)
            raise AssertionError("set_fixed_sites went through beside %s" % stem)
        except EpvError as e:
            assert str(e) == ("epv error 4: epv_set_fixed_sites: %s would count across fixed sites: switch that layer "
                              "off (epv_set_%s with 0) first" % (name, stem)), str(e)
        assert d.fixed_sites() == 0
        d.set_fixed_sites(np.zeros(fp.n_sites, np.uint8))      # an empty mask holds nothing
        getattr(d, "enable_" + stem)(*off)
    d.close()
    return dict(layers=len(REFUSING))


def run_layers(spec):
    """the five per-site layers, on with regions: their read-outs are their references over the sampled paths"""
    import bevents_ref
    import mixing_ref
    import origin_ref
    import patterns_ref
    import pavg_ref
    model, tree, fp, cap = inputs(spec)
    n, P, K = fp.n_sites, 5, 3
    mask = host.region_fixed_mask(n, spec["layout"])
    d = context(spec, model, tree, fp, cap, mask)
    d.enable_path_average(P)
    d.enable_branch_events(True)
    d.enable_lineage_origins(True)
    d.enable_change_patterns(True)
    d.enable_mixing(K)
    d.reset()
    pa, be, pt = 0, 0, 0
    origin, age = 0, 0
    m = mixing_ref.Mixing(n, K)
    for w in range(3):
        d.sweep(1, SEED, sweep_base=w)
        for stem in ("path_average", "branch_events", "lineage_origins", "change_patterns", "mixing"):
            getattr(d, "accumulate_" + stem)()
        p = d.paths()
        pa = pa + pavg_ref.counts(p, tree.branches, P)
        be = be + bevents_ref.counts(p)
        pt = pt + patterns_ref.counts(p, tree)
        o1, a1 = origin_ref.sample(p, tree)
        origin, age = origin + o1.astype(np.uint64), age + a1
        m.sample(p, linked=w > 0)
    assert d.path_average(counts=True)[0] == 3 and np.array_equal(d.path_average(counts=True)[1], pa)
    assert np.array_equal(d.branch_events(counts=True)[1], be)
    assert np.array_equal(d.change_patterns(counts=True)[1], pt)
    ns, rows, got_origin, got_age = d.lineage_origins(counts=True)
    assert ns == 3 and np.array_equal(got_origin, origin) and np.array_equal(got_age, age)
    for got, want in zip(d.mixing(counts=True), m.counts()):
        assert np.array_equal(np.asarray(got), np.asarray(want))
    assert not m.moved[mask != 0].any() and m.moved[mask == 0].any()      # a fixed site never moves
    d.close()
    return dict(samples=3)


if __name__ == "__main__":
    spec = json.loads(sys.argv[1])
    out = {"row": run_row, "default": run_default, "decoupling": run_decoupling, "lifetime": run_lifetime,
           "group": run_group, "refusing": run_refusing, "layers": run_layers, "cpp": run_cpp, "cli": run_cli}[spec["kind"]](spec)
    print("ok " + json.dumps(out))
