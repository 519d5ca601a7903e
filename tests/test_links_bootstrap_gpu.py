"""graal_end_links_bootstrap on the GPU: the data's own columns word for word those of graal_end_links; a replicate word for word what
graal_end_links returns on a fresh engine that holds the resampled counts (the defining test); every replicate equal to the numpy
restatement (tests/link_boot_reference.py) outside the cells a near-boundary draw excuses; the statistics and the mutual counts exactly
those of the returned matrix; deterministic and independent of n_rep and of the batching; refused where graal_end_links is; free of side
effects on a run; sensible on a simulated genome cut into shuffled pieces; and written by the command line as support_table gives it."""
import ctypes
import functools
import mmap
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from graal_amd import em, links, synth
from graal_amd.lib import Engine, GraalError, LINK_VALID, _i32p, _i64p
from tests import junction_boot_reference as BR
from tests import link_boot_reference as KR
from tests import link_reference as LR
from tests.test_junctions_gpu import _layout
from tests.test_links_gpu import engine_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [pytest.param(*c, id="%s-%d-%d-%d" % c) for c in KR.SMALL_CASES]
STATS = ("support", "mutual", "q_sum", "q_min", "q_max")
DATA = ("end_a", "end_b", "q", "contacts", "status")


def tol(A):
    return 1e-9 * np.asarray(A, np.float64) + 1           # tests/test_links_gpu.py's bound, in Q


@functools.lru_cache(maxsize=None)
def gpu(name, quirk, min_frags, seed):
    """One engine per case: graal_end_links, then the bootstrap of N_REP replicates twice, of 5, of 1, without the matrix, and at a
    threshold taken from the matrix."""
    e = engine_for(KR.small_case(name), quirk=quirk)
    try:
        out = {"links": e.end_links_q(min_frags)}
        out["full"] = e.end_links_bootstrap_q(seed, KR.N_REP, min_frags, 0, replicates=True)
        out["again"] = e.end_links_bootstrap_q(seed, KR.N_REP, min_frags, 0, replicates=True)
        out["five"] = e.end_links_bootstrap_q(seed, 5, min_frags, 0, replicates=True)
        out["one"] = e.end_links_bootstrap_q(seed, 1, min_frags, 0, replicates=True)
        out["plain"] = e.end_links_bootstrap_q(seed, KR.N_REP, min_frags, 0)
        m = len(out["full"]["q"])
        out["threshold"] = int(out["full"]["q_rep"][3, m // 2])
        out["at_threshold"] = e.end_links_bootstrap_q(seed, KR.N_REP, min_frags, out["threshold"], replicates=True)
        out["other_seed"] = e.end_links_bootstrap_q(seed + 1, 5, min_frags, 0, replicates=True)
        out["links_after"] = e.end_links_q(min_frags)
    finally:
        e.close()
    return out


@pytest.mark.parametrize("name,quirk,min_frags,seed", CASES)
def test_data_columns_are_end_links(name, quirk, min_frags, seed):
    g = gpu(name, quirk, min_frags, seed)
    for k in ("full", "five", "one", "plain", "at_threshold", "other_seed"):
        for col, want in zip(DATA, g["links"]):
            assert np.array_equal(g[k][col], want) and g[k][col].dtype == want.dtype, (k, col)
    for x, y in zip(g["links"], g["links_after"]):
        assert np.array_equal(x, y)
    assert len(g["links"][0]) >= 10 and (g["links"][4] == LINK_VALID).all()


@pytest.mark.parametrize("name,quirk,min_frags,seed", CASES)
def test_a_replicate_is_end_links_on_the_resampled_counts(name, quirk, min_frags, seed):
    """The defining test.  For three replicates (the first, one behind a batch boundary, the last): the same layout in a fresh engine
    with the restatement's resampled counts, graal_end_links there, exact int64 equality with the bootstrap's row on every cell no
    flagged draw excuses.  graal_upload_contacts refuses a count of 0, so the contacts that drew 0 are left out of the fresh engine's
    list: a term of count 0 is exactly 0, so no listed link's score moves, but a link whose every contact inside the window drew 0 is
    not listed there -- the fresh table is a subset of the data's and is compared on all of its rows (the rest of the row is compared
    with the numpy restatement in test_replicates_equal_restatement: DEFINING_REPS are among REF_REPS).  At r = 0
    graal_end_links_best on the fresh engine names the links the bootstrap of one replicate counts as mutual."""
    P = KR.small_case(name)
    G = gpu(name, quirk, min_frags, seed)
    g = G["full"]
    B = KR.small_boot(name, quirk, min_frags)
    assert np.array_equal(g["end_a"], B.end_a) and np.array_equal(g["end_b"], B.end_b)
    for r in KR.DEFINING_REPS:
        counts, flags = BR.draw_counts(B.R.row, B.R.col, B.R.count, seed, r)
        flagged = np.array([bool(flags[s[t != 0.0]].any()) for s, t in zip(B.sel, B.t)])
        keep = counts > 0
        P2 = dict(P)
        for k, v in (("coo_row", B.R.row), ("coo_col", B.R.col), ("coo_val", counts.astype(np.float32))):
            P2[k] = np.asarray(v)[keep]
        assert np.array_equal(P2["coo_val"].astype(np.int64), counts[keep]) and (~keep).sum() >= 5
        e = engine_for(P2, quirk=quirk)
        try:
            a, b, q, _, st = e.end_links_q(min_frags)
            best = e.end_links_best(min_frags)[2] if r == 0 else None
        finally:
            e.close()
        key = g["end_a"].astype(np.int64) << 32 | g["end_b"]
        at = np.searchsorted(key, a.astype(np.int64) << 32 | b)
        assert (at < len(key)).all() and np.array_equal(key[at], a.astype(np.int64) << 32 | b)      # a subset of the data's links
        assert len(a) >= 10 and len(a) >= 0.6 * len(key) and (st == LINK_VALID).all()
        fl = flagged[at]
        assert flagged.sum() <= 0.02 * len(key) + 1
        assert np.array_equal(q[~fl], g["q_rep"][r][at][~fl]), (r, int((q != g["q_rep"][r][at])[~fl].sum()))
        if best is not None:
            one = G["one"]
            assert np.array_equal(one["q_rep"][0], g["q_rep"][0])
            ga, gb = g["end_a"].tolist(), g["end_b"].tolist()
            want = set(zip(best[0].tolist(), best[1].tolist()))
            got = np.array([(x, y) in want for x, y in zip(ga, gb)])
            listed = np.zeros(len(key), bool)
            listed[at] = True
            row = g["q_rep"][0]
            if not flagged.any():
                # the fresh engine chooses among the links it lists: numpy's rule on the bootstrap's row over those links, exactly
                assert np.array_equal(got, KR.mutual_counts(ga, gb, row[None, :], listed) == 1)
            # ... and where no end's choice hangs on a flagged link or on one the fresh engine does not list, the two calls agree
            every, fresh = KR.best_partners(ga, gb, row, np.ones(len(key), bool)), KR.best_partners(ga, gb, row, listed)
            dirty = set(g["end_a"][flagged].tolist()) | set(g["end_b"][flagged].tolist())
            same = lambda x: x not in dirty and every.get(x) == fresh.get(x)
            clean = np.array([same(x) and same(y) for x, y in zip(ga, gb)])
            assert np.array_equal(one["mutual"][clean] == 1, got[clean]) and set(np.unique(one["mutual"]).tolist()) <= {0, 1}
            assert clean.sum() >= 0.5 * len(key) and (got & clean).sum() >= 1


@pytest.mark.parametrize("name,quirk,min_frags,seed", CASES)
def test_replicates_equal_restatement(name, quirk, min_frags, seed):
    g = gpu(name, quirk, min_frags, seed)["full"]
    B = KR.small_boot(name, quirk, min_frags)
    L, A, flagged, st = KR.small_replicates(name, quirk, min_frags, seed)
    assert np.array_equal(g["status"], st[0]) and (st == KR.VALID).all()
    rep = g["q_rep"][list(KR.REF_REPS)]
    assert rep.shape == L.shape
    cells = ~flagged
    assert cells.sum() >= 0.98 * B.m * len(KR.REF_REPS)
    excess = np.abs(rep - L)[cells] / tol(A[cells])
    print("%s quirk %d min_frags %d: %d cells, %d flagged, largest |q_rep - L*| / tolerance %.3e"
          % (name, quirk, min_frags, cells.sum(), flagged.sum(), float(excess.max())))
    assert (excess <= 1).all(), int((excess > 1).sum())
    # the replicates differ from the data's own scores and from each other: the draws are in them (a link on one contact of count 1
    # redraws that count about one time in three)
    assert (rep[0] != g["q"]).mean() > 0.6 and (rep[0] != rep[1]).mean() > 0.6


@pytest.mark.parametrize("name,quirk,min_frags,seed", CASES)
def test_statistics_are_those_of_the_matrix(name, quirk, min_frags, seed):
    G = gpu(name, quirk, min_frags, seed)
    for k, thr in (("full", 0), ("at_threshold", G["threshold"]), ("five", 0), ("one", 0)):
        g = G[k]
        ok = g["status"] == LINK_VALID
        rep = g["q_rep"]
        assert np.array_equal(g["support"], np.where(ok, (rep > thr).sum(axis=0), 0)), k
        assert np.array_equal(g["q_sum"], np.where(ok, rep.sum(axis=0), 0)), k
        assert np.array_equal(g["q_min"], np.where(ok, rep.min(axis=0), 0)), k
        assert np.array_equal(g["q_max"], np.where(ok, rep.max(axis=0), 0)), k
        assert np.array_equal(g["mutual"], KR.mutual_counts(g["end_a"], g["end_b"], rep, ok, thr)), k
        assert g["support"].dtype == np.int32 and g["mutual"].dtype == np.int32 and (g["mutual"] <= g["support"]).all()
    full = G["full"]
    assert (full["mutual"] > 0).any()
    if name != "circ":                                    # (the ring case has one join the data prefer; the others have competing ones)
        assert (full["mutual"] > 0).sum() >= 3 and (full["mutual"] < full["support"]).any()


@pytest.mark.parametrize("name,quirk,min_frags,seed", CASES)
def test_deterministic_whatever_n_rep_and_threshold(name, quirk, min_frags, seed):
    G = gpu(name, quirk, min_frags, seed)
    full = G["full"]
    for k in full:
        assert np.array_equal(full[k], G["again"][k]), k
    for k in DATA + STATS:
        assert np.array_equal(full[k], G["plain"][k]), k
    assert "q_rep" not in G["plain"]
    # N_REP spans three batches, the last one short: its first five rows are the call of five
    assert KR.N_REP > 2 * 64 and KR.N_REP % 64 != 0
    assert np.array_equal(G["five"]["q_rep"], full["q_rep"][:5])
    assert np.array_equal(G["at_threshold"]["q_rep"], full["q_rep"])
    assert (G["other_seed"]["q_rep"] != G["five"]["q_rep"]).mean() > 0.6
    # a threshold at one replicate's value moves the support by exactly the replicates between 0 and it
    thr = G["threshold"]
    lo, hi = min(0, thr), max(0, thr)
    between = ((full["q_rep"] > lo) & (full["q_rep"] <= hi)).sum(axis=0) * (1 if thr > 0 else -1)
    assert thr != 0 and np.array_equal(full["support"] - G["at_threshold"]["support"], between)
    assert (full["support"] != G["at_threshold"]["support"]).any()


def test_float_columns_and_table():
    name, quirk, min_frags, seed = KR.SMALL_CASES[1]
    G = gpu(name, quirk, min_frags, seed)["five"]
    e = engine_for(KR.small_case(name), quirk=quirk)
    try:
        f = e.end_links_bootstrap(seed, 5, min_frags, replicates=True)
        t = links.support_table(e, seed, 5, min_frags)
        plain = links.link_table(e, min_frags)
    finally:
        e.close()
    Qs = float(1 << 30)
    assert np.array_equal(f["end_a"], G["end_a"]) and np.array_equal(f["status"], G["status"])
    assert np.array_equal(f["support"], G["support"] / 5.0) and np.array_equal(f["mutual"], G["mutual"] / 5.0)
    assert ((f["mutual"] >= 0) & (f["mutual"] <= f["support"]) & (f["support"] <= 1)).all()
    assert np.array_equal(f["mean"], G["q_sum"] / 5.0 / Qs) and np.array_equal(f["min"], G["q_min"] / Qs)
    assert np.array_equal(f["max"], G["q_max"] / Qs) and np.array_equal(f["replicates"], G["q_rep"] / Qs)
    assert np.array_equal(f["score"], G["q"] / Qs)
    assert tuple(t) == links.SUPPORT_COLUMNS
    for c in links.COLUMNS:
        assert np.array_equal(t[c], plain[c]), c
    assert np.array_equal(t["support"], f["support"]) and np.array_equal(t["mutual"], f["mutual"])
    assert np.array_equal(t["boot_mean"], f["mean"]) and np.array_equal(t["boot_min"], f["min"]) and np.array_equal(t["boot_max"], f["max"])


def test_no_side_effect_on_a_run():
    """run_em with end_links_bootstrap_q() called at the end of every cycle and in the middle of one gives the same accepted moves and
    likelihoods (tests/test_links_gpu.py's pattern)."""
    from tests.test_sampler_gpu import make_gpu_sampler
    P = synth.with_dense(synth.make_problem(n_bins=70, nnz=1200, n_sub=1, seed=41, contig_weights=(5, 4, 3), mean_len_bp=2000.0,
                                            param=synth.make_param_simu(fact=200.0, v_inter=0.02), grid_bp=2000))
    n = P["n_frags"]
    runs = []
    for call in (False, True):
        rng = np.random.RandomState(5)
        smp = make_gpu_sampler(P, rng, reference_arithmetic="exact")
        seen, calls = [], []

        def on_step(j, i, trace, smp=smp, seen=seen, call=call, calls=calls):
            seen.append(i)
            if call and (len(seen) % n == 0 or len(seen) == n // 2):
                calls.append(smp.engine.end_links_bootstrap_q(3, 5, 1, 0, replicates=True))

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs)))
        smp.free_gpu()
        assert (len(calls) >= 3) == call
    (m0, l0, c0), (m1, l1, c1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1)


def test_refusals():
    name, quirk, min_frags, seed = KR.SMALL_CASES[3]
    P = KR.small_case(name)
    want = gpu(name, quirk, min_frags, seed)["five"]
    e = engine_for(P)
    try:
        seg = mmap.mmap(-1, max(e.exchange_bytes(2), mmap.PAGESIZE))   # (rank 0 of two: a world of one has no exchange)
        e.attach_exchange(seg, 0, 2, 0)
        with pytest.raises(GraalError, match=r"one rank.*code 3\)"):
            e.end_links_bootstrap_q(seed, 5, min_frags)
        e.detach_exchange()
        for n_rep in (0, 1025, -1):
            with pytest.raises(GraalError, match=r"n_rep.*code 1\)"):
                e.end_links_bootstrap_q(seed, n_rep, min_frags, 0, replicates=True)
        with pytest.raises(GraalError, match=r"min_frags.*code 1\)"):
            e.end_links_bootstrap_q(seed, 5, 0)
        assert e._L.graal_end_links_bootstrap(e._h, 1, ctypes.c_uint64(seed), 5, 0, 0, None) == 1
        # the fetch: no result yet (the refused calls left none), then the matrix only after a call that wanted it, then cap
        m = len(want["q"])
        i32 = lambda: np.zeros(m, np.int32)
        i64 = lambda: np.zeros(m, np.int64)
        a, b, sup, mut = i32(), i32(), i32(), i32()
        q, c, s, lo, hi = i64(), i64(), i64(), i64(), i64()
        st = np.zeros(m, np.uint8)
        rep = np.zeros((5, m), np.int64)
        p32, p64 = (lambda x: x.ctypes.data_as(_i32p)), (lambda x: x.ctypes.data_as(_i64p))
        fetch = lambda rp, cap, sp=sup: e._L.graal_end_links_bootstrap_fetch(
            e._h, p32(a), p32(b), p64(q), p64(c), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None if sp is None else p32(sp),
            p32(mut), p64(s), p64(lo), p64(hi), None if rp is None else p64(rp), cap)
        assert fetch(None, m) == 3 and "first" in e._L.graal_last_error(e._h).decode()
        e.end_links_bootstrap_q(seed, 5, min_frags, 0)
        assert fetch(rep, m) == 1 and "want_rep" in e._L.graal_last_error(e._h).decode() and not rep.any()
        assert fetch(None, m - 1) == 1 and "cap" in e._L.graal_last_error(e._h).decode()
        assert fetch(None, m, None) == 1
        assert fetch(None, m) == 0 and np.array_equal(sup, want["support"]) and np.array_equal(mut, want["mutual"])
        e.end_links_q(min_frags)                                        # a later graal_end_links ends the bootstrap's result
        assert fetch(None, m) == 3
        got = e.end_links_bootstrap_q(seed, 5, min_frags, 0, replicates=True)     # the engine works afterwards
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.end_links_bootstrap_q(1, 5)
    finally:
        e.close()


@pytest.mark.parametrize("seed,weakest", [(2024, 64), (7, 63)])
def test_simulated_genome_true_adjacencies_are_the_mutual_links(seed, weakest):
    """tests/test_links_gpu.py's simulated genome (1,000 bins in 4 chromosomes cut into shuffled, partly reversed pieces of 80 bins),
    64 replicates under resampling seed 77: the true adjacencies' mean mutual fraction exceeds that of every listed link that is not
    one, and a link whose smallest replicate is positive is supported by all 64.  Every true adjacency is mutual in at least the
    weakest count measured (one MI355X: 64 / 64 under simulation seed 2024, 63 / 64 under seed 7; the results are bit-identical from call
    to call, so the measured value is the bound, less nothing).  The other figures: DESIGN.md section 8d2."""
    R = 64
    par = synth.make_param_simu(fact=1500.0, v_inter=0.5)
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(4, 3, 2, 1), param=par)
    s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
    rng = np.random.RandomState(seed)
    pieces = []
    for c, frags in LR.contig_lists(s).items():
        pieces += [frags[i:i + 80] for i in range(0, len(frags), 80)]
    true = set()
    flip = rng.rand(len(pieces)) < 0.5

    def end_of(p, tail):      # the end of piece p that was its original head (tail=False) or tail, in the shuffled layout
        f = pieces[p][-1][0] if tail else pieces[p][0][0]
        return 2 * f + (int(tail) if not flip[p] else 1 - int(tail))
    for p in range(len(pieces) - 1):
        if s["id_c"][pieces[p][0][0]] == s["id_c"][pieces[p + 1][0][0]]:
            true.add(tuple(sorted((end_of(p, True), end_of(p + 1, False)))))
    shuffled = [[(f, -o) for f, o in reversed(pieces[p])] if flip[p] else pieces[p] for p in rng.permutation(len(pieces))]
    cut = LR.layout(s["len_bp"], shuffled)
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.set_params(par)
        e.upload_frags(s)
        r, c, v = e.simulate_contacts(seed)
        e.upload_contacts(r, c, v)
        e.upload_frags(cut)
        g = e.end_links_bootstrap_q(77, R, 1, 0)
    finally:
        e.close()
    ok = g["status"] == LINK_VALID
    is_true = np.array([(int(x), int(y)) in true for x, y in zip(g["end_a"], g["end_b"])])
    assert ok.all() and is_true.sum() == len(true) == len(pieces) - 4 and (~is_true).sum() > 0
    Qs = float(1 << 30)
    print("seed %d: %d links, %d true adjacencies: mutual mean %.4f, smallest %d / %d, support smallest %d / %d, smallest replicate %.1f; "
          "other links: mutual largest %d / %d, support largest %d / %d, largest replicate %.1f"
          % (seed, len(ok), is_true.sum(), g["mutual"][is_true].mean() / R, g["mutual"][is_true].min(), R, g["support"][is_true].min(), R,
             g["q_min"][is_true].min() / Qs, g["mutual"][~is_true].max(), R, g["support"][~is_true].max(), R, g["q_max"][~is_true].max() / Qs))
    assert g["mutual"][is_true].min() >= weakest, (int(g["mutual"][is_true].min()), weakest)
    assert g["mutual"][is_true].mean() > g["mutual"][~is_true].max()
    sure = g["q_min"] > 0
    assert sure.sum() >= 3 and (g["support"][sure] == R).all()
    assert (g["support"][g["q_max"] <= 0] == 0).all() and (g["mutual"] <= g["support"]).all()


def test_run_writes_link_support_tsv():
    """The rows are support_table's of the layout the run ended in (rebuilt from junctions.tsv: its fragments, orientations and order
    are in those rows), on a sampler built from the same dataset the way graal_amd.run builds its own, with the run's --seed for the
    resampling.  The contig labels are the run's own and are not compared."""
    from graal_amd import pyramid as pyr
    from graal_amd.sampler import sampler
    P = synth.make_problem(n_bins=300, nnz=3000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    par = synth.make_param_simu(fact=300.0, v_inter=0.02)
    with tempfile.TemporaryDirectory() as d:
        data, out = os.path.join(d, "data"), os.path.join(d, "out")
        synth.write_dataset(P, data)
        cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
               "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--junctions", "--links", "--link-support", "16",
               "--links-min-frags", "2", "--no-fit", "--param", *[str(float(x)) for x in par]]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(os.path.join(out, "link_support.tsv")).read().splitlines()
        plain = open(os.path.join(out, "links.tsv")).read().splitlines()
        junc = [l.split("\t") for l in open(os.path.join(out, "junctions.tsv")).read().splitlines()[1:]]
        root = os.path.join(data, "pyramids", "pyramid_1_thresh_auto")
        inp = pyr.simulation_inputs(pyr.Pyramid(root, 1), 0, candidates_blacklist=[0], allow_repeats=False)
    assert lines[0].split("\t") == list(links.SUPPORT_COLUMNS)
    rows = [l.split("\t") for l in lines[1:]]
    nc = len(links.COLUMNS)
    assert len(rows) == len(plain) - 1 > 0 and [x[:nc] for x in rows] == [l.split("\t") for l in plain[1:]]
    n = int(inp["n_frags"])
    members = {}
    for x in junc:
        members.setdefault(int(x[0]), []).append(x)
    contigs = [[(int(x[2]), int(x[4])) for x in m] + [(int(m[-1][3]), int(m[-1][5]))] for _, m in sorted(members.items())]
    in_rows = {f for fr in contigs for f, _ in fr}
    contigs += [[(f, 1)] for f in range(n) if f not in in_rows]
    smp = sampler(True, inp["S_o_A_frags"], inp["collector_id_repeats"], inp["frag_dispatcher"], inp["id_frag_duplicated"],
                  inp["id_frags_blacklisted"], inp["n_frags"], inp["n_new_frags"], inp["init_n_sub_frags"], inp["n_new_sub_frags"],
                  None, inp["hic_matrix_sub_sampled"], inp["np_sub_frags_len_bp"], inp["np_sub_frags_id"], inp["np_sub_frags_accu"],
                  inp["mean_squared_frags_per_bin"], inp["norm_vect_accu"], inp["S_o_A_sub_frags"], inp["hic_matrix"],
                  inp["mean_value_trans"], 1, False, None, device=0, rng=np.random.RandomState(3), reference_arithmetic="exact")
    try:
        smp.set_param_simu(np.asarray(par, dtype=np.float32))
        smp.engine.upload_frags(_layout(np.asarray(inp["S_o_A_frags"]["len_bp"]), contigs))
        t = links.support_table(smp, 3, 16, 2)
    finally:
        smp.free_gpu()
    for j, c in enumerate(links.SUPPORT_COLUMNS):
        if c in ("contig_a", "contig_b"):
            continue
        got = np.array([float(x[j]) for x in rows])
        assert np.array_equal(got, np.asarray(t[c], np.float64), equal_nan=True), c
    assert ((t["mutual"] >= 0) & (t["mutual"] <= t["support"]) & (t["support"] <= 1)).all()
    assert (t["support"] * 16 == np.rint(t["support"] * 16)).all()
