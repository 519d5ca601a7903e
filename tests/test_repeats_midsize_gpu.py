"""GPU: repeated bins at mid-size shapes (tests/repeat_cases.py; tests/test_repeat_cases_cpu.py shows what the cases hold) against the
dense oracle: k_rep_full over 7 to 15 blocks and k_rep_delta over up to 141, every row of its per-block sums (K = 10), bins with four and
five fragments, two repeated bins that are neighbours in id, the last bin repeated, observed counts in every branch of lik_double --
next to the short-contig flow, next to the late stage's finishers (k_fin in the default arithmetic, the tiled kernels in the
reference's), and at one sub-fragment per bin.

Tolerances: rel 1e-8 on the full likelihood; on a candidate delta 1e-7 |logL| on grid coordinates in the default arithmetic and
2e-9 |logL| in the reference's (repeat_cases.tolerance).  One mispriced pixel is worth 0.2 to 30 units, the tolerances 3e-4 to 2e-2.
Measured on an MI355X: full likelihood within 8.5e-11 relative, deltas within 4.6e-12 |logL| in every case.

What these cases found: at one sub-fragment per bin, k_fin's shortcut for a fragment pair's mass priced a copy of a repeated bin (no
sub-fragments in the sparse path) as a fragment with one -- a contig beyond what k_tm prices itself, holding a copy, had that copy's mass
counted twice (1.2e-4 |logL|, 14 units, in the 600-bin case; the small cases never leave k_tm).  The shortcut now skips such pairs."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import repeat_cases as RC
from tests import util

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("name,variant", RC.CASES)


def engine_for_case(name, variant, s, max_id):
    e = RC.engine(name, variant, s)
    assert e.relabel_contigs() == max_id
    return e


@CASES
def test_full_likelihood(name, variant):
    """eval_full against DenseOracle.evaluate, and again after one inactive copy is switched on in the layout uploaded: the sum moves by
    that copy's worth."""
    P, D = RC.problem(name, variant), RC.dense(name, variant)
    s, max_id = RC.layout(name, variant)
    f = RC.layout_kinds(P, s)["lone_inactive"][0]
    e = engine_for_case(name, variant, s, max_id)
    try:
        want = D.evaluate(s)
        got = e.eval_full()
        print(name, variant, "full: rel", abs(got - want) / abs(want))
        assert got == pytest.approx(want, rel=1e-8)
        s2 = O.copy_state(s)
        s2["activ"][f] = 1
        e.upload_frags(s2)
        assert e.relabel_contigs() == max_id
        want2 = D.evaluate(s2)
        got2 = e.eval_full()
        assert abs(want2 - want) > 1e-6 * abs(want)
        assert got2 == pytest.approx(want2, rel=1e-8)
    finally:
        e.close()


@CASES
def test_candidate_deltas(name, variant):
    """All 13 x K candidates of every proposal against oracle_deltas_with_repeats."""
    s, max_id = RC.layout(name, variant)
    r = RC.oracle_results(name, variant)
    tol = RC.tolerance(variant, r["base"])
    e = engine_for_case(name, variant, s, max_id)
    try:
        got = [e.eval_candidates(fA, fBs, max_id) for _kind, fA, fBs in RC.proposals(name, variant)]
    finally:
        e.close()
    err = [np.abs(g - w).max() / abs(r["base"]) for g, w in zip(got, r["want"])]
    print(name, variant, "deltas: largest |got - want| / |logL| per proposal", ["%.2e" % x for x in err], "allowed %.0e" % (tol / abs(r["base"])))
    for (kind, fA, fBs), g, w in zip(RC.proposals(name, variant), got, r["want"]):
        assert g.shape == w.shape == (len(fBs), 13)
        bad = np.argwhere(~(np.abs(g - w) <= tol))
        assert len(bad) == 0, (kind, fA, fBs, len(bad), bad[:6].tolist(), (g - w)[tuple(bad[0])], tol)


@CASES
def test_rows_do_not_depend_on_their_company(name, variant):
    """A neighbour's 13 scores are a fixed function of its int64 sums: evaluated alone, or with the neighbours in the opposite order,
    they are the same 64-bit words.  (A wrong k, per_k or s_acc index across k_rep_delta's blocks puts a pixel into another row.)"""
    s, max_id = RC.layout(name, variant)
    props = RC.proposals(name, variant)
    e = engine_for_case(name, variant, s, max_id)
    try:
        for kind, fA, fBs in (props[1], props[3]):
            both = e.eval_candidates(fA, fBs, max_id)
            assert np.abs(both).max() > 0
            back = e.eval_candidates(fA, fBs[::-1], max_id)
            assert np.array_equal(back[::-1].view(np.int64), both.view(np.int64)), (kind, np.argwhere(back[::-1] != both)[:6].tolist())
            for k, fB in enumerate(fBs):
                alone = e.eval_candidates(fA, [fB], max_id)
                assert np.array_equal(alone[0].view(np.int64), both[k].view(np.int64)), (kind, k, fB, alone[0] - both[k])
    finally:
        e.close()


@CASES
def test_commits(name, variant):
    """Two commits, one behind the other: an inactive copy is switched on (op 8), then the oracle's best candidate of the copy inside the
    longest contig.  After each, the layout downloaded behind begin_step is the oracle's candidate, relabelled, field by field, and the
    full likelihood is the oracle's of that layout.  (Not delta == after - before: for a pixel of two repeated bins the reference's
    candidate score is not the true difference -- comment in k_rep_delta -- and the engine follows the reference.)"""
    from tests.test_engine_gpu import relabel_ref
    D = RC.dense(name, variant)
    s, max_id = RC.layout(name, variant)
    props = RC.proposals(name, variant)
    want1 = RC.oracle_results(name, variant)["want"][1]
    k, op = np.unravel_index(np.argmax(want1), want1.shape)
    moves = [(props[2][1], props[2][2][0], 8), (props[1][1], props[1][2][k], int(op))]
    assert s["activ"][moves[0][0]] == 0 and s["rep"][moves[1][0]] == 1
    e = engine_for_case(name, variant, s, max_id)
    try:
        for fA, fB, op in moves:
            want, stale = util.oracle_candidate(s, fA, fB, op, max_id)
            assert not stale
            assert any(not np.array_equal(want[f], s[f]) for f in O.FIELDS)
            want_max = relabel_ref(want)
            assert e.apply_move(fA, fB, op, max_id) == 0
            _stats, got_max = e.begin_step()
            got = e.download_frags()
            assert got_max == want_max
            for f in O.FIELDS:
                assert np.array_equal(got[f], want[f]), (fA, fB, op, f)
            assert e.eval_full() == pytest.approx(D.evaluate(want), rel=1e-8), (fA, fB, op)
            s, max_id = want, want_max
        assert s["activ"][moves[0][0]] == 1
    finally:
        e.close()


def test_short_run_matches_the_oracle():
    """24 steps of step_max_likelihood over originals, copies and ordinary fragments of the 320-bin problem in reference arithmetic, the
    same fragment ids and seed on both sides: accepted moves, statistics, likelihood series and final layout.  (The oracle's side takes
    4 s on the CPU; tests/test_repeat_cases_cpu.py asserts that it swaps an activity and moves a copy.)"""
    from tests.test_sampler_gpu import make_gpu_sampler
    want = RC.oracle_run()
    P = RC.problem(RC.RUN["name"], RC.RUN["variant"])
    rng = np.random.RandomState(RC.RUN["seed"])
    g = make_gpu_sampler(P, rng, reference_arithmetic="strict")
    try:
        g.init_likelihood()
        trace, lik, stats = [], [], []
        for i in RC.RUN["ids"]:
            r = g.step_max_likelihood(int(i), RC.RUN["delta"])
            trace.append((int(i), int(r[6]), int(r[5])))
            lik.append(float(r[0]))
            stats.append((int(r[1]), int(r[2]), int(r[4]), float(r[7])))
        assert trace == want["trace"]
        assert stats == want["stats"]
        assert np.allclose(lik, want["likelihood"], rtol=1e-8, atol=0)
        g.gpu_vect_frags.copy_from_gpu()
        for f in O.FIELDS:
            assert np.array_equal(getattr(g.gpu_vect_frags, f), want["final"][f]), f
    finally:
        g.free_gpu()
