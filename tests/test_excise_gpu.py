"""graal_block_excisions on the GPU: equal to the brute-force restatement (tests/excise_reference.py) on the small windowed problems with
the mode flag off and on, consistent with full evaluations of the excised layouts, with the junction scores (a head or tail span is a
plain cut) and with the insertion scores of the excised layout (an excision is the inverse of an insertion); its refusals, determinism
and freedom from side effects on a run; graal_amd.excise's rounds on a simulated genome with misplaced runs, followed by the insertion
rounds that put them back; and the run module's tables."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from graal_amd import em, excise, scaffold, synth
from graal_amd.lib import EXCISE_CIRCULAR, EXCISE_VALID, EXCISE_WHOLE, INSERT_VALID, JUNCTION_VALID, GraalError
from oracle.sparse_numpy import SparseScorer
from tests import excise_reference as XR
from tests import link_reference as LR
from tests import window_cases
from tests.test_excise_cpu import long_runs
from tests.test_scaffold_gpu import assert_true_chromosomes, engine_for, simulated

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, q) for n in ("w1", "w3") for q in (False, True)]

_CASES, _REFS = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = LR.case(name) if name == "circ" else window_cases.small(name)
    return _CASES[name]


def span_sets(s):
    """The tilings up to 4 fragments, runs of 10, 17 and 30 fragments, then one call with every linear contig of >= 2 fragments whole
    and, in a ring, two spans."""
    sets = list(excise.tilings(s, None, 4)) + [long_runs(s)]
    circ = np.asarray(s["circ"])
    first, last = [], []
    for m in LR.contigs_of(s).values():
        if circ[m[0]] == 1:
            first += [m[0], m[3]]; last += [m[1], m[3]]
        elif len(m) >= 2:
            first.append(m[0]); last.append(m[-1])
    sets.append((np.array(first, np.int32), np.array(last, np.int32)))
    return sets


def reference(name, quirk):
    """The brute-force restatement of span_sets, once per (problem, mode)."""
    if (name, quirk) not in _REFS:
        P = case(name)
        R = XR.restatement(P, quirk=quirk)
        _REFS[name, quirk] = [R.excisions(P["S_o_A_frags"], first, last) for first, last in span_sets(P["S_o_A_frags"])]
    return _REFS[name, quirk]


@pytest.mark.parametrize("name,quirk", CASES + [("circ", True)])
def test_equals_reference(name, quirk):
    P = case(name)
    s = P["S_o_A_frags"]
    pos, lc = np.asarray(s["pos"]), np.asarray(s["l_cont"])
    sets = span_sets(s)
    e = engine_for(P, quirk=quirk)
    try:
        got = [e.block_excisions_q(first, last) for first, last in sets]
    finally:
        e.close()
    seen = set()
    for (first, last), (q, c, st), (rq, rc, rst, A) in zip(sets, got, reference(name, quirk)):
        assert np.array_equal(st, rst) and np.array_equal(c, rc)
        if len(first):
            print(name, quirk, len(first), "spans: max |q - rq|", int(np.max(np.abs(q - rq))), "max A", int(A.max()))
        assert np.all(np.abs(q - rq) <= 1e-9 * A + 1), (q - rq, A)
        seen |= set(st.tolist())
        v = st == EXCISE_VALID
        seen |= {"head"} if (v & (pos[first] == 0)).any() else set()
        seen |= {"tail"} if (v & (pos[last] == lc[last] - 1)).any() else set()
        seen |= {"one"} if (v & (first == last)).any() else set()
        seen |= {"long"} if (v & (pos[last] - pos[first] >= 29)).any() else set()
        seen |= {"scored"} if (v & (q != 0) & (c > 0)).sum() >= 5 else set()
    want = {EXCISE_VALID, EXCISE_WHOLE, "head", "tail", "one", "scored"} | ({EXCISE_CIRCULAR} if name == "circ" else {"long"})
    assert want <= seen, seen


def test_the_mode_moves_the_score_of_mixed_bins_only():
    """w3 has bins of mixed RF counts, reversed: the trans price of X x rest uses the indexing, so some span's q differs with the mode
    on; w1 (one sub-fragment per bin) has none: the same integers."""
    for name, moved in (("w1", False), ("w3", True)):
        a = np.concatenate([r[0] for r in reference(name, False)])
        b = np.concatenate([r[0] for r in reference(name, True)])
        assert (a != b).any() == moved


def _noise(sp, s, S, first, last):
    """What the float32 re-centring moves in the full likelihood and E leaves out: the pairs inside X, inside L and inside R, and every
    bin's own sub-fragment pairs (tests/test_flips_gpu._noise's construction)."""
    m, sl = XR._members(s, first, last)
    masks = []
    for g in (m[sl], m[:sl.start], m[sl.stop:]):
        k = np.zeros(len(s["id_c"]), bool); k[g] = True
        masks.append(k)
    own = lambda x: sp.full(x) - sp.full(x, same_bin=False)
    return sum(abs(sp.restricted(S, k) - sp.restricted(s, k)) for k in masks) + abs(own(S) - own(s))


@pytest.mark.parametrize("name,quirk", [("w3", False), ("w3", True), ("w1", False)])
def test_sampled_spans_equal_full_evaluation_difference(name, quirk):
    """E = eval_full(excised layout, uploaded as the restatement builds it) - eval_full(layout) for ~15 spans, within the re-centring
    noise (the flips' tolerance)."""
    P = case(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    sets = list(excise.tilings(s, None, 4)) + [long_runs(s)]
    first, last = np.concatenate([a for a, _ in sets]), np.concatenate([b for _, b in sets])
    e = engine_for(P, quirk=quirk)
    try:
        E = np.concatenate([e.block_excisions(a, b)[0] for a, b in sets])
        assert np.isfinite(E).all()
        e.relabel_contigs()
        base = e.eval_full()
        for i in np.unique(np.linspace(0, len(first) - 1, 15).astype(int)):
            S = XR.excise_layout(s, int(first[i]), int(last[i]))
            noise = _noise(sp, s, S, int(first[i]), int(last[i]))
            e.upload_frags(S)
            e.relabel_contigs()
            want = e.eval_full() - base
            assert abs(E[i] - want) <= 1.5 * noise + 1e-6 * max(1.0, abs(want)), (first[i], last[i], E[i], want, noise)
        e.upload_frags(s)
    finally:
        e.close()


@pytest.mark.parametrize("name,quirk", CASES)
def test_head_and_tail_spans_are_plain_cuts(name, quirk):
    """A span at the head or at the tail of its contig: E = -(graal_junction_scores at the one junction it cuts), to 1e-9 A + 1 with the
    restatement's A (the junction call sums a pair with its lower slot outer, the excision with X's fragment outer)."""
    P = case(name)
    s = P["S_o_A_frags"]
    calls = []
    for w in (1, 2, 9, 15):                                           # (the head and the tail span of the shortest contig stay disjoint)
        first, last, junc = [], [], []
        for m in LR.contigs_of(s).values():
            first += [m[0], m[-w]]; last += [m[w - 1], m[-1]]; junc += [m[w - 1], m[-w - 1]]
        calls.append((np.array(first, np.int32), np.array(last, np.int32), np.array(junc)))
    e = engine_for(P, quirk=quirk)
    try:
        J, jst = e.junction_scores_q()
        got = [e.block_excisions_q(first, last) for first, last, _ in calls]
    finally:
        e.close()
    W = XR.window(P, quirk=quirk)
    for (first, last, junc), (q, c, st) in zip(calls, got):
        A = W.excisions(s, first, last)[3]
        assert (st == EXCISE_VALID).all() and (jst[junc] == JUNCTION_VALID).all() and (q != 0).all()
        assert np.all(np.abs(q + J[junc]) <= 1e-9 * A + 1), (q, J[junc])


@pytest.mark.parametrize("name,quirk", CASES)
def test_the_excised_piece_goes_back_at_minus_the_score(name, quirk):
    """After edit_layout(*excise_edit(...)) of spans with both flanks, insertions() lists (X, L.tail, rev 0) with score -E, to the same
    bound, wherever the edit's canonical order kept the contig's direction and the candidate is listed."""
    P = case(name)
    s = P["S_o_A_frags"]
    first, last = list(excise.tilings(s, None, 3))[3]
    prev, nxt = np.asarray(s["prev"]), np.asarray(s["next"])
    k = np.nonzero((prev[first] >= 0) & (nxt[last] >= 0))[0][::6]     # (far enough apart to be excised together: a few per contig)
    first, last = first[k], last[k]
    A = XR.window(P, quirk=quirk).excisions(s, first, last)[3]
    e = engine_for(P, quirk=quirk)
    n_checked = 0
    try:
        for i in range(len(first)):
            e.upload_frags(s)
            q, c, st = e.block_excisions_q(first[i:i + 1], last[i:i + 1])
            e.edit_layout(*excise.excise_edit(s, first[i:i + 1], last[i:i + 1]))
            now = e.download_frags()
            assert XR.chains(now) == XR.chains(XR.excise_layout(s, first[i], last[i]))
            p, f, r, iq, ic, ist = e.insertions_q(3)
            hit = np.nonzero((p == first[i]) & (f == prev[first[i]]) & (r == 0))[0]
            if len(hit) and now["next"][prev[first[i]]] == nxt[last[i]]:
                assert st[0] == EXCISE_VALID and ist[hit[0]] == INSERT_VALID
                assert abs(int(q[0]) + int(iq[hit[0]])) <= 1e-9 * A[i] + 1, (first[i], last[i], int(q[0]), int(iq[hit[0]]))
                n_checked += 1
    finally:
        e.close()
    assert n_checked >= 3


def test_refusals_leave_outputs_layout_and_state_alone():
    P = case("w3")
    s = P["S_o_A_frags"]
    lists = LR.contigs_of(s)
    big = max(lists.values(), key=len)
    other = min((m for m in lists.values() if m[0] != big[0]), key=lambda m: m[0])
    n = len(s["id_c"])
    from graal_amd.lib import _i32p, _i64p
    u8 = ctypes.POINTER(ctypes.c_uint8)
    e = engine_for(P, quirk=True)
    try:
        before = e.download_frags()
        good = (np.array([big[0], big[3]], np.int32), np.array([big[1], big[5]], np.int32))
        want = e.block_excisions_q(*good)
        bad = {"overlaps": ([big[0], big[4], big[2]], [big[1], big[6], big[5]], 2),      # span 2 = positions 2..5 meets span 1 = 4..6
               "overlaps ": ([big[1], big[2], big[0]], [big[2], big[3], big[6]], 1),   # span 1 meets span 0 before the long span 2 comes
               "two contigs": ([big[0], big[2]], [big[1], other[0]], 1),
               "before first": ([big[3]], [big[1]], 0),
               "out of range": ([big[0], n], [big[1], n], 1),
               "out of range ": ([-1], [big[1]], 0)}
        for why, (first, last, k) in bad.items():
            first, last = np.array(first, np.int32), np.array(last, np.int32)
            q = np.full(len(first), 7, np.int64); c = np.full(len(first), 7, np.int64); st = np.full(len(first), 9, np.uint8)
            rc = e._L.graal_block_excisions(e._h, len(first), first.ctypes.data_as(_i32p), last.ctypes.data_as(_i32p), q.ctypes.data_as(_i64p),
                                            c.ctypes.data_as(_i64p), st.ctypes.data_as(u8))
            msg = e._L.graal_last_error(e._h).decode()
            assert rc == 1 and why.strip() in msg and "span %d" % k in msg, (why, rc, msg)
            assert (q == 7).all() and (c == 7).all() and (st == 9).all()
        with pytest.raises(GraalError, match="overlaps"):
            e.block_excisions([big[0], big[0]], [big[1], big[1]])
        assert all(len(x) == 0 for x in e.block_excisions_q([], []))
        after = e.download_frags()
        for k in LR.FIELDS:
            assert np.array_equal(after[k], before[k]), k
        for u, v in zip(want, e.block_excisions_q(*good)):      # (a refusal leaves the next call unaffected)
            assert np.array_equal(u, v)
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.block_excisions([0], [1])
    finally:
        e.close()


def test_deterministic_in_any_span_order_and_for_an_unsorted_contact_list():
    P = case("w3")
    s = P["S_o_A_frags"]
    first, last = list(excise.tilings(s, None, 3))[0]                 # (every fragment a span: a contact feeds many closing sums)
    perm = np.random.RandomState(4).permutation(len(first))
    e = engine_for(P, quirk=True)
    try:
        want = e.block_excisions_q(first, last)
        again = e.block_excisions_q(first, last)
        shuffled = e.block_excisions_q(first[perm], last[perm])
        cp = np.random.RandomState(3).permutation(len(P["coo_row"]))
        e.upload_contacts(np.asarray(P["coo_row"])[cp], np.asarray(P["coo_col"])[cp], np.asarray(P["coo_val"])[cp])
        unsorted = e.block_excisions_q(first, last)
    finally:
        e.close()
    assert len(first) >= 100 and np.count_nonzero(want[0]) >= 100
    for u, v, w, x in zip(want, again, shuffled, unsorted):
        assert np.array_equal(u, v) and np.array_equal(u[perm], w) and np.array_equal(u, x)


def test_no_side_effect_on_a_run():
    """run_em with block_excisions() of every fragment of the current layout (its first tiling) called at the end of every cycle and in
    the middle of one, each call followed by a refused call (an overlap), gives the same accepted moves and likelihoods: neither the
    call nor a refusal touches the step state (carried total, pending correction, proposal tables) or draws from the generator."""
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
                e = smp.engine
                sets = list(excise.tilings(e.download_frags(), None, 2))
                if sets:
                    first, last = sets[0]
                    E, c, st = e.block_excisions(first, last)
                    assert len(E) == len(first) and set(st.tolist()) <= {EXCISE_VALID}
                    calls.append(len(E))
                    with pytest.raises(GraalError, match="overlaps"):        # (a refusal in the middle of a run, too)
                        e.block_excisions(first[[0, 0]], last[[0, 0]])

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs), rng.randint(1 << 30), len(calls)))
        smp.free_gpu()
    (m0, l0, c0, r0, _), (m1, l1, c1, r1, n_calls) = runs
    assert n_calls >= 3
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1) and r0 == r1


def spurious_and_planted(e, s):
    """On the engine's own simulated list (fetched again: the draw is a function of layout, tables, parameters and seed): the largest
    score of an excision of the TRUE layout `s` -- by the windowed restatement over the single fragments, by the engine over the
    complete tilings up to 3 --, the gains of the planted excisions by the restatement, and the restatement's insertion scores of the
    freed runs at their true homes (rev 0) in the layout with every run excised."""
    par = synth.make_param_simu(fact=1500.0, v_inter=0.5)
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(4, 3, 2, 1), param=par)   # (simulated()'s genome)
    P["coo_row"], P["coo_col"], P["coo_val"] = e.simulate_contacts(2024)
    P["param_simu"] = par
    W = XR.window(P)
    spurious = max(W.excisions(s, *x)[0].max() / LR.Q for x in excise.tilings(s, None, 1))
    e.upload_frags(s)
    spurious_gpu = max(np.nanmax(e.block_excisions(*x)[0]) for x in excise.tilings(s, None, 3))
    bad, first, last = XR.planted(s)
    gains = W.excisions(bad, first, last)[0] / LR.Q
    freed = XR.excise_layout(s, first, last)
    home = W.insertion_scores(freed, first, np.asarray(s["prev"])[first], np.zeros(len(first), np.int64))[0] / LR.Q
    return spurious, spurious_gpu, gains, home


def test_excise_then_insert_relocates_misplaced_runs():
    """The scaffold tests' genome with the six runs of tests/excise_reference.PLANTS (1 to 3 fragments) moved into other chromosomes
    or more than two windows from home: excise_rounds(min_score=20) makes every planted run a contig of its own and its recorded logL
    never falls; scaffold(insert_max_frags=3) afterwards puts every run back between its true neighbours, at a logL not below the
    scrambled layout's.  The rounds also cut a chromosome where a run is missing (the gap it left is a weak junction, and a unit next
    to one is a span): scaffold's joins close those again around the returned run.  min_score must sit between two figures on the list
    this test scores, and the test asserts that first, on the engine's own list (seed 2024), and prints them.  On contacts drawn by
    numpy (seed 5) the best excision of the true layout up to 3 fragments scores -66.5, the six planted runs gain 200.0 to 1,544.8,
    and the windowed restatements alone (excisions, links and insertions behind the same drivers) end on the true layout at the true
    layout's logL."""
    e, s = simulated()
    try:
        spurious, spurious_gpu, gains, home = spurious_and_planted(e, s)
        print("largest spurious excision %.2f (one fragment, restatement) %.2f (<= 3 fragments, engine), planted gains %s, insertion scores "
              "at home %s" % (spurious, spurious_gpu, np.round(gains, 1).tolist(), np.round(home, 1).tolist()))
        assert spurious < 20.0 < gains.min() and spurious_gpu < 20.0 and home.min() > 0, (spurious, spurious_gpu, gains, home)
        bad, first, last = XR.planted(s)
        with pytest.raises(AssertionError):
            assert_true_chromosomes(bad, s)
        e.upload_frags(bad)
        rec = excise.excise_rounds(e, max_frags=3, min_score=20.0)
        freed = e.download_frags()
        rec2 = scaffold.scaffold(e, insert_max_frags=3)
        got = e.download_frags()
    finally:
        e.close()
    print("excise rounds", [(r["round"], r["excisions"], r["contigs"], round(r["logL"], 1), r["kept"]) for r in rec])
    print("scaffold rounds", [(r["round"], r["cuts"], r["joins"], r["contigs"], round(r["logL"], 1), r["kept"]) for r in rec2])
    logl = [r["logL"] for r in rec]
    assert len(rec) >= 2 and all(r["kept"] == 1 for r in rec) and all(b > a for a, b in zip(logl, logl[1:])), rec
    pieces = {tuple(sorted(m.tolist())) for m in LR.contigs_of(freed).values()}
    assert all(tuple(range(int(f), int(l) + 1)) in pieces for f, l in zip(first, last)), sorted(p for p in pieces if len(p) <= 3)
    assert all(r["kept"] == 1 for r in rec2) and rec2[-1]["logL"] >= rec[0]["logL"], rec2
    assert_true_chromosomes(got, s)


def test_run_excise_and_excisions_write_their_tables(tmp_path):
    """--excise writes its rounds, --excisions the score table of the tilings of the final layout: every run of up to
    --excise-max-frags fragments that is not its whole contig, once, with a score wherever the status is valid."""
    P = synth.make_problem(n_bins=300, nnz=30000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    par = synth.make_param_simu(fact=300.0, v_inter=0.02)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    synth.write_dataset(P, data)
    cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
           "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--excise", "--excisions", "--excise-max-frags", "2",
           "--excise-min-score", "1.0", "--no-fit", "--param", *[repr(float(x)) for x in par]]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(os.path.join(out, "excise.tsv")).read().splitlines()
    assert lines[0].split("\t") == list(excise.ROUND_COLUMNS) and lines[1].split("\t")[:2] == ["0", "0"]
    lines = open(os.path.join(out, "excisions.tsv")).read().splitlines()
    assert lines[0].split("\t") == list(excise.COLUMNS)
    rows = [l.split("\t") for l in lines[1:]]
    ix = {c: i for i, c in enumerate(excise.COLUMNS)}
    assert len(rows) > 0 and all(1 <= int(x[ix["frags"]]) <= 2 for x in rows)
    assert len({(x[0], x[1]) for x in rows}) == len(rows)
    assert all((x[ix["score"]] != "nan") == (int(x[ix["status"]]) == EXCISE_VALID) for x in rows)
    assert sum(int(x[ix["status"]]) == EXCISE_VALID for x in rows) > 0
