"""graal_ring_scores and graal_close_rings on the GPU: equal to the numpy restatement (tests/ring_reference.py) and to the engine's own
full evaluations, unaffected by the trans-branch indexing, deterministic, free of side effects on a run, exact when committed, right on
simulated data, and reachable from scaffold() and the command line."""
import mmap
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from graal_amd import em, rings, scaffold, synth
from graal_amd.lib import (EDIT_SAME_CONTIG, GraalError, RING_CLOSE, RING_NONFINITE, RING_OPEN, RING_SINGLE)
from tests import edit_reference as ER
from tests import junction_reference as JR
from tests import ring_reference as RR
from tests.engine_states import cached, engine_for
from tests.link_reference import FIELDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = float(1 << 30)
SMALL = ("sub3", "sub1", "circ")


def problem(name):
    return cached(("rings", name), lambda: JR.case(name))


def reference(name):
    def run():
        parts = {}
        return RR.ring_scores_windowed(problem(name), parts=parts) + (parts,)
    return cached(("rings-windowed", name), run)


def contigs_of(s):
    return [(int(c), np.nonzero(s["id_c"] == c)[0]) for c in np.unique(s["id_c"])]


def assert_equals(got, want):
    q, c, st = got
    R, C, St, A = want[:4]
    assert np.array_equal(st, St) and np.array_equal(c, C)
    scored = St <= RING_OPEN
    assert (q[~scored] == 0).all()
    err = np.abs(q[scored] - R[scored])
    assert np.all(err <= 1e-9 * A[scored] + 1), float(err.max())


@pytest.mark.parametrize("name", SMALL)
def test_equals_reference_and_ignores_the_mode_flag(name):
    P = problem(name)
    e = engine_for(P)
    try:
        off = e.ring_scores_q()
        e.set_mode(ref_trans_accu=True)
        on = e.ring_scores_q()
    finally:
        e.close()
    assert_equals(off, reference(name))
    for a, b in zip(off, on):
        assert np.array_equal(a, b)
    assert (off[2] == RING_CLOSE).sum() >= 10
    if name == "circ":
        assert (off[2][P["S_o_A_frags"]["circ"] == 1] == RING_OPEN).all()


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("circ", False), ("circ", True)])
def test_equals_the_engines_full_evaluation_of_the_toggled_layout(name, quirk):
    """R / 2^30 = eval_full(toggled) - eval_full(current) within 1e-9 A / 2^30 + 2^-30 (terms + 1), for every scored contig."""
    P = problem(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    _, _, St, A, parts = reference(name)
    e = engine_for(P, quirk=quirk)
    try:
        q, _, st = e.ring_scores_q()
        e.relabel_contigs()
        base = e.eval_full()
        checked = 0
        for c, m in contigs_of(s):
            f = int(m[0])
            if st[f] > RING_OPEN:
                continue
            e.upload_frags(RR.toggle(s, c))
            e.relabel_contigs()
            want = e.eval_full() - base
            tol = 1e-9 * A[f] / Q + (parts["terms"][f] + 1) / Q
            print(name, quirk, c, len(m), q[f] / Q, want, abs(q[f] / Q - want), tol)
            assert abs(q[f] / Q - want) <= tol, (c, q[f] / Q, want, tol)
            checked += 1
        assert checked >= 2
    finally:
        e.close()


def test_exploded_genome_is_all_single():
    P = problem("sub1")
    e = engine_for(P)
    try:
        e.explode()
        q, c, st = e.ring_scores_q()
    finally:
        e.close()
    assert (st == RING_SINGLE).all() and (q == 0).all()


def near_wrap_problem(fact):
    """sub1 with the first five bins of its last contig (one sub-fragment each, ~3 kb together: far shorter than the 80 kb window) a ring
    of their own whose first and last fragments are 1 bp long: their centres lie 1 bp apart across the wrap, s_tot - s = 0.001 kb.  The
    ring price of that pair is (n / nmax)^slope ~ 4e4 times its linear price of ~3e-3 fact: with fact 2e7 past the 2^31 a term may hold,
    and the contig is NONFINITE (whatever the other contigs are at that scale)."""
    P = dict(JR.case("sub1"))
    par = synth.make_param_simu(fact=fact, v_inter=0.05, d_max=80.0)
    s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
    c = int(s["id_c"].max())
    m = np.nonzero(s["id_c"] == c)[0]
    m = m[np.argsort(s["pos"][m])]
    sub_len = np.array(P["np_sub_frags_len_bp"], dtype=np.float32, copy=True).reshape(-1, 3)
    for f in (m[0], m[4]):
        s["len_bp"][f] = 1
        sub_len[f, 0] = np.float32(0.001)
    s["start_bp"][m] = np.cumsum(s["len_bp"][m]) - s["len_bp"][m]
    s["l_cont_bp"][m] = s["len_bp"][m].sum()
    s = ER.edit(s, cuts=[int(m[4])])[0]
    P["np_sub_frags_len_bp"] = sub_len.reshape(np.shape(P["np_sub_frags_len_bp"]))
    P["S_o_A_frags"] = RR.toggle(s, c)
    P["param_simu"] = par
    assert s["l_cont"][m[0]] == 5 and s["l_cont_bp"][m[0]] / 1000.0 < 0.1 * float(par[5])
    return P, m[:5]


@pytest.mark.parametrize("fact", (2000.0, 2e7))
def test_ring_shorter_than_the_window_with_a_pair_at_the_wrap(fact):
    P, m = near_wrap_problem(fact)
    want = RR.ring_scores_windowed(P)
    e = engine_for(P)
    try:
        got = e.ring_scores_q()
    finally:
        e.close()
    print(fact, int(want[2][m[0]]), want[0][m[0]] / Q, got[0][m[0]] / Q)
    assert_equals(got, want)
    if fact == 2e7:
        assert want[2][m[0]] == RING_NONFINITE
    else:
        assert want[2][m[0]] == RING_OPEN


def test_deterministic_and_round_trip():
    P = problem("circ")
    e = engine_for(P)
    try:
        a = e.ring_scores_q()
        b = e.ring_scores_q()
        soa = e.download_frags()
        e.upload_frags(soa)
        c = e.ring_scores_q()
    finally:
        e.close()
    for x in (b, c):
        for u, v in zip(a, x):
            assert np.array_equal(u, v)


def test_no_side_effect_on_a_run():
    """run_em with ring_scores() called at the end of every cycle and in the middle of one gives the same accepted moves, likelihoods and
    generator state."""
    from tests.test_sampler_gpu import make_gpu_sampler
    P = synth.with_dense(synth.make_problem(n_bins=70, nnz=1200, n_sub=1, seed=41, contig_weights=(5, 4, 3), mean_len_bp=2000.0,
                                            param=synth.make_param_simu(fact=200.0, v_inter=0.02), grid_bp=2000))
    n = P["n_frags"]
    runs = []
    for call in (False, True):
        rng = np.random.RandomState(5)
        smp = make_gpu_sampler(P, rng, reference_arithmetic="exact")
        seen = []

        def on_step(j, i, trace, smp=smp, seen=seen, call=call):
            seen.append(i)
            if call and (len(seen) % n == 0 or len(seen) == n // 2):
                smp.engine.ring_scores()

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs), rng.get_state()))
        smp.free_gpu()
    (m0, l0, c0, g0), (m1, l1, c1, g1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1)
    assert np.array_equal(g0[1], g1[1]) and g0[2:] == g1[2:]


def same_layout(a, b):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), k


def test_close_rings_equals_reference_and_cut_at_the_wrap_undoes_it():
    P = problem("sub3")
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    cs = [m[np.argsort(s["pos"][m])] for _, m in contigs_of(s)]
    frags = [int(cs[0][0]), int(cs[2][len(cs[2]) // 2])]
    want, _ = RR.close(s, frags)
    e = engine_for(P)
    try:
        st = e.close_rings(frags)
        assert (st == 0).all()
        got = e.download_frags()
        same_layout(got, want)
        e.edit_layout(cuts=[int(cs[0][-1]), int(cs[2][-1])])
        same_layout(e.download_frags(), s)
        same_layout(ER.edit(want, cuts=[int(cs[0][-1]), int(cs[2][-1])])[0], s)
        # the refusal this call stands next to is unchanged
        with pytest.raises(GraalError) as err:
            e.edit_layout(joins=[(2 * int(cs[0][0]), 2 * int(cs[0][-1]) + 1)])
        assert list(err.value.status) == [EDIT_SAME_CONTIG]
    finally:
        e.close()


def test_close_rings_refusals_leave_the_layout_alone():
    P = problem("circ")
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    n = len(s["pos"])
    ring = next(m for _, m in contigs_of(s) if s["circ"][m[0]] == 1)
    lin = next(m for _, m in contigs_of(s) if s["circ"][m[0]] != 1)
    # the linear contig's tail cut off: a one-fragment contig
    single = ER.edit(s, cuts=[int(lin[np.argsort(s["pos"][lin])][-2])])[0]
    one = int(np.nonzero(single["l_cont"] == 1)[0][0])
    e = engine_for(P, single)
    try:
        for frags in ([n], [-1], [int(lin[0]), int(ring[0])], [one], [int(lin[0]), int(lin[1])], [int(lin[0]), one, n]):
            want, st_want = RR.close(single, frags)
            assert want is None
            with pytest.raises(GraalError, match=r"code 1\)") as err:
                e.close_rings(frags)
            assert np.array_equal(err.value.status, st_want), frags
            same_layout(e.download_frags(), single)
        assert len(e.close_rings([])) == 0
        same_layout(e.download_frags(), single)
    finally:
        e.close()


@pytest.mark.parametrize("name", SMALL)
def test_closing_every_scored_contig_at_once_adds_the_scores_exactly(name):
    P = problem(name)
    s = P["S_o_A_frags"]
    _, _, St, A, parts = reference(name)
    e = engine_for(P)
    try:
        q, _, st = e.ring_scores_q()
        heads = [int(m[0]) for _, m in contigs_of(s) if st[m[0]] == RING_CLOSE]
        assert len(heads) >= 1
        e.relabel_contigs()
        before = e.eval_full()
        e.close_rings(heads)
        e.relabel_contigs()
        after = e.eval_full()
        gain = sum(int(q[f]) for f in heads) / Q
        tol = sum(1e-9 * A[f] / Q + (parts["terms"][f] + 1) / Q for f in heads)
        print(name, len(heads), after - before, gain, abs(after - before - gain), tol)
        assert abs((after - before) - gain) <= tol
        # and the closed layout scores the opening as minus the closure, bit for bit
        q2, _, st2 = e.ring_scores_q()
        assert (st2[heads] == RING_OPEN).all() and np.array_equal(q2[heads], -q[heads])
    finally:
        e.close()


def test_repeats_and_ranks_refused():
    P = problem("sub1")
    e = engine_for(P)
    try:
        seg = mmap.mmap(-1, max(e.exchange_bytes(2), mmap.PAGESIZE))   # (rank 0 of two: a world of one has no exchange)
        e.attach_exchange(seg, 0, 2, 0)
        with pytest.raises(GraalError, match="one rank"):
            e.ring_scores()
        with pytest.raises(GraalError, match="one rank"):
            e.close_rings([0])
        e.detach_exchange()
        e.ring_scores()
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.ring_scores()
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.close_rings([0])
    finally:
        e.close()


# ---- end to end, on contacts the engine simulates from a truth ---------------------------------------------------------------------
def truth_engine(seed=7):
    """The engine holding case 'circ' (a ring of 30 bins, a linear contig of 15) with contacts simulated from it, and the truth."""
    P = problem("circ")
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    from graal_amd.lib import Engine
    e = Engine(0)
    e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                      P["mean_squared_frags_per_bin"])
    e.set_params(P["param_simu"])
    e.upload_frags(s)
    r, c, v = e.simulate_contacts(seed)
    e.upload_contacts(r, c, v)
    return e, s


def neighbour_pairs(s, frags):
    return {frozenset((int(f), int(s["next"][f]))) for f in frags if s["next"][f] >= 0}


def test_close_rings_closes_exactly_the_true_rings():
    e, s = truth_engine()
    try:
        ring = np.nonzero(s["circ"] == 1)[0]
        opened = s
        for c, m in contigs_of(s):
            if s["circ"][m[0]] == 1:
                opened = RR.toggle(opened, c)
                want = RR.toggle(opened, c)      # (the truth with the ring's head and tail linked, as a closure writes them)
        e.upload_frags(opened)
        rec = rings.close_rings(e)
        print({k: rec[k] for k in rings.RECORD_COLUMNS}, rec["tolerance"])
        assert rec["closed"] == 1 and rec["opened"] == 0 and rec["kept"] == 1
        assert abs((rec["logL"] - rec["logL_before"]) - rec["expected_gain"]) <= rec["tolerance"] and rec["expected_gain"] > 0
        got = e.download_frags()
        for k in FIELDS:
            if k != "id_c":               # (close_rings relabels)
                assert np.array_equal(got[k], want[k]), k
        assert (got["circ"][ring] == 1).all() and got["circ"].sum() == len(ring)
        # nothing left to do; and with open_rings the true ring stays closed
        rec = rings.close_rings(e, open_rings=True)
        assert rec["closed"] == 0 and rec["opened"] == 0
    finally:
        e.close()


def test_scaffold_closes_the_true_ring():
    """The truth cut into pieces: the ring opened at its wrap, the linear contig cut in three.  scaffold() rejoins the linear contig,
    its rounds settle, and close_rings_min_score closes the ring.  The ring is cut at its wrap only: a join is priced by the LINEAR
    model, and the reference's ring price is not a small change of it (about s_eff^slope times the linear price at s_eff = s (s_tot - s)
    / s_tot kb), so contacts drawn from a true ring make joins between its pieces score near zero or below -- with the sparse numpy
    scorer on this truth (seed 7) the joins of its halves gain -93.5 and -237.6, those of its thirds -25.0, +238.0 and -237.0, while
    the two joins of the linear contig gain +940.3 and +1,235.4.  Closing is scored by the ring model itself: +35,695.9."""
    e, s = truth_engine()
    try:
        ring = np.nonzero(s["circ"] == 1)[0]
        ring = ring[np.argsort(s["pos"][ring])]
        lin = np.nonzero(s["circ"] != 1)[0]
        lin = lin[np.argsort(s["pos"][lin])]
        want_ring, want_lin = neighbour_pairs(RR.toggle(RR.toggle(s, int(s["id_c"][ring[0]])), int(s["id_c"][ring[0]])), ring), neighbour_pairs(s, lin)
        e.edit_layout(cuts=[int(ring[-1]), int(lin[4]), int(lin[9])])
        cut = e.download_frags()
        assert cut["circ"].sum() == 0 and len(np.unique(cut["id_c"])) == 4
        record = scaffold.scaffold(e, close_rings_min_score=0.0)
        got = e.download_frags()
        print([(r["round"], r["cuts"], r["joins"], r["contigs"], r["logL"], r["kept"]) for r in record])
        assert (got["circ"][ring] == 1).all() and (got["circ"][lin] == 0).all()
        assert len(np.unique(got["id_c"])) == 2 and got["l_cont"][ring[0]] == len(ring) and got["l_cont"][lin[0]] == len(lin)
        assert neighbour_pairs(got, ring) == want_ring and len(want_ring) == len(ring) and neighbour_pairs(got, lin) == want_lin
        assert record[-1]["joins"] == 1 and record[-1]["cuts"] == 0 and record[-1]["kept"] == 1 and record[-1]["logL"] > record[-2]["logL"]
        assert record[-1]["round"] == record[-2]["round"] + 1 and sum(r["joins"] for r in record[:-1]) == 2
        # the default changes nothing: on the settled layout no row is added, and none without the parameter
        assert len(scaffold.scaffold(e)) == 1
        rows = scaffold.scaffold(e, close_rings_min_score=0.0)
        assert len(rows) == 2 and rows[-1]["joins"] == 0 and rows[-1]["kept"] == 1 and rows[-1]["logL"] == rows[0]["logL"]
    finally:
        e.close()


def test_run_writes_circularise_and_rings_tsv():
    P = synth.make_problem(n_bins=300, nnz=3000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    with tempfile.TemporaryDirectory() as d:
        data, out = os.path.join(d, "data"), os.path.join(d, "out")
        synth.write_dataset(P, data)
        cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
               "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--circularise", "--rings",
               "--no-fit", "--param", *[str(float(x)) for x in synth.make_param_simu(fact=300.0, v_inter=0.02)]]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(os.path.join(out, "circularise.tsv")).read().splitlines()
        assert lines[0].split("\t") == list(rings.RECORD_COLUMNS) and len(lines) == 2
        rec = dict(zip(rings.RECORD_COLUMNS, lines[1].split("\t")))
        assert int(rec["kept"]) in (0, 1) and int(rec["closed"]) >= 0
        lines = open(os.path.join(out, "rings.tsv")).read().splitlines()
        assert lines[0].split("\t") == list(rings.COLUMNS)
        rows = [dict(zip(rings.COLUMNS, l.split("\t"))) for l in lines[1:]]
        import re
        n_contigs = int(re.search(r"steps in .*?: (\d+) contigs", r.stdout).group(1))
        assert len(rows) == n_contigs and n_contigs <= sum(int(x["frags"]) for x in rows) <= 300   # (the pyramid filters some bins out)
        assert all(int(x["status"]) in (RING_CLOSE, RING_OPEN, RING_SINGLE, RING_NONFINITE) for x in rows)
        # what --circularise closed is a ring in the table, and no linear contig left scores above the threshold
        assert sum(int(x["circ"]) for x in rows) >= int(rec["closed"]) * int(rec["kept"])
        if int(rec["kept"]):
            assert all(not float(x["score"]) > 0 for x in rows if int(x["status"]) == RING_CLOSE)
