"""GPU: every kernel that prices a pair, under contact-model parameters that are NOT the synthetic default (kuhn 1, lm 9.6, slope -1.5,
d 3) -- the sets of tests/param_cases.py: two fitted ones (a Kuhn length that is not 1 takes rippe's division branch and moves every
parameter-only factor of rippe_circ and of rings.h's precomputed copy), d - 2 negative, d - 2 zero.  A fit (rippe_fit) starts every
run without --no-fit from such a set, and the nuisance steps send one to a live handle behind every MCMC step.

(a) the full evaluation and the candidate deltas against outputs RECORDED from the reference's own kernels under these sets
    (tests/golden/ref_likelihood_params.npz), as tests/test_ref_kernels_gpu.py does under the default;
(b) every flow of a candidate evaluation (tests/step_plan_cases.py) bit for bit against k_strict_dense, and -- k_strict_dense has no
    anchor of its own under these sets -- against the dense oracle;
(c) the whole-layout scorers, the maps, a committed ring closure and the simulator against their numpy restatements;
(d) the own-pixel carry along a run;
(e) parameter changes on ONE used handle (the window shrinks below, then grows beyond, everything allocated so far): every call equals
    the same call as the first on a fresh handle created with those parameters;
(f) the sampler with nuisance-parameter steps from a fitted start, against the oracle;
(g) graal_set_params's refusals, which leave the parameters in force and every result alone.

Every tolerance is the one the suite already uses for the same quantity under the default set (named next to each test); each test
prints its worst |engine - reference| / tolerance (DESIGN.md section 7 records them).  The preconditions of tests/param_cases.py --
the set is not the default, the reference is finite and not all zero, no pair reaches the fixed point's 2^31, no NONFINITE status, each
test's own floor of cases -- are asserted in front of the launches."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from graal_amd import em, excise, flips
from graal_amd.lib import (EXCISE_VALID, FLIP_VALID, INSERT_VALID, JUNCTION_NONFINITE, JUNCTION_VALID, LINK_VALID, RING_CLOSE, RING_NONFINITE,
                           RING_OPEN, SWAP_VALID, GraalError)
from oracle import oracle as O
from tests import excise_reference as XR
from tests import flip_reference as FR
from tests import insert_reference as IR
from tests import junction_reference as JR
from tests import link_reference as LR
from tests import map_reference as MR
from tests import param_cases as PC
from tests import ref_cases as C
from tests import ring_reference as RR
from tests import sim_reference as SIM
from tests import step_plan_cases as SC
from tests import swap_reference as SR
from tests import window_cases as WC
from tests.engine_states import cached, engine_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
LIK = np.load(os.path.join(HERE, "golden", "ref_likelihood_params.npz"))
Q = float(1 << 30)
RECORDED = [(li, name) for li in C.PARAM_LAYOUT_INDEX for name in PC.NAMES]
RECORDED_IDS = ["%s-%s" % (C.LAYOUTS[li]["name"], name) for li, name in RECORDED]


def tol_q(A):
    """The layout scorers' bound, in Q: 1e-9 of the sum of |terms|, + 1 for the rounding of the sum."""
    return 1e-9 * np.asarray(A, np.float64) + 1


def report(family, what, params, err, tol):
    worst = PC.worst_ratio(err, tol)
    print("\n[params] %s | %s | %s: worst |engine - reference| / tolerance = %.3g" % (family, what, params, worst))
    return worst


# ---- (a) the recorded reference ------------------------------------------------------------------------------------------------------
def recorded(li, params):
    lay = C.layout_under(li, params)
    PC.assert_not_default(lay["P"]["param_simu"])
    assert int(LIK[C.param_key(li, params, "digest")]) == lay["digest"], "the regenerated inputs are not the recorded ones"
    total, deltas = float(LIK[C.param_key(li, params, "total")]), LIK[C.param_key(li, params, "deltas")]
    PC.assert_reference_usable(total, (lay["name"], params))
    PC.assert_reference_usable(deltas[~np.isnan(deltas)], (lay["name"], params))
    return lay, total, deltas


@pytest.mark.parametrize("li,params", RECORDED, ids=RECORDED_IDS)
def test_a_full_evaluation_equals_the_recorded_reference(li, params):
    """rel 1e-8 (tests/test_ref_kernels_gpu.py)."""
    from tests.test_ref_kernels_gpu import engine_of
    lay, want, _ = recorded(li, params)
    e = engine_of(lay)
    got = e.eval_full()
    e.close()
    report("a", "full " + lay["name"], params, abs(got - want), 1e-8 * abs(want))
    assert got == pytest.approx(want, rel=1e-8)


@pytest.mark.parametrize("li,params", RECORDED, ids=RECORDED_IDS)
def test_a_candidate_deltas_equal_the_recorded_reference(li, params):
    """2e-9 |logL|, 1e-7 |logL| with repeated bins (tests/test_ref_kernels_gpu.py); a neighbour equal to fA scores 0 for all 13
    candidates although the reference prices them: both halves asserted."""
    from tests.test_ref_kernels_gpu import MUT, engine_of
    lay, base, deltas_f = recorded(li, params)
    assert deltas_f.shape == (len(lay["proposals"]), C.K, C.N_OPS)
    tol = (1e-7 if lay["repeats"] else 2e-9) * abs(base)
    _, _, st_f = C.recorded_candidates(MUT, li)          # (the candidates' layouts do not depend on the parameters)
    e = engine_of(lay)
    worst, n_self, n_compared = 0.0, 0, 0
    for i, (fA, fBs) in enumerate(lay["proposals"]):
        got = e.eval_candidates(fA, fBs, lay["max_id"])
        for k, fB in enumerate(fBs):
            if fB == fA:
                assert np.all(got[k] == 0), (fA, got[k])
                assert np.all(np.isfinite(deltas_f[i, k][[0, 1, 8]])), (fA, deltas_f[i, k])
                assert np.array_equal(np.isnan(deltas_f[i, k]), st_f[i * C.K + k] > 0)
                n_self += 1
                continue
            assert not np.any(np.isnan(deltas_f[i, k])), "only a candidate of fA with itself is stale in the reference"
            err = np.abs(got[k] - deltas_f[i, k])
            worst = max(worst, float(err.max()) / tol)
            n_compared += err.size
            assert np.all(err <= tol), (lay["name"], params, fA, fB, err.max(), tol, got[k] - deltas_f[i, k])
    e.close()
    assert n_compared >= 6 * C.N_OPS
    print("\n[params] a | deltas %s | %s: worst |engine - reference| / tolerance = %.3g (%d compared, %d neighbours equal to fA)" %
          (lay["name"], params, worst, n_compared, n_self))


# ---- (b) every flow of a candidate evaluation ----------------------------------------------------------------------------------------
ORACLE_ANCHORED = ("contigs of at most 16", "contigs of about 40", "late stage: two contigs of 260", "repeated bins")
SMALLEST = ("contigs of at most 16", "repeated bins")         # the two that also run under d_below_2 and d_is_2
FLOWS = [(name, p) for name in SC.STRICT for p in PC.FITTED] + [(name, p) for name in SMALLEST for p in ("d_below_2", "d_is_2")]
EXACT = "exact arithmetic, a contig of 1,100"


@pytest.fixture(scope="module")
def dense_kernel(tmp_path_factory):
    """k_strict_dense's scores of FLOWS, from two child processes (GRAAL_STRICT_DENSE=1 is read once per process)."""
    out = {}
    names = list(SC.CASES)
    for which, sets in (("strict", PC.FITTED), (",".join(str(names.index(n)) for n in SMALLEST), ("d_below_2", "d_is_2"))):
        path = str(tmp_path_factory.mktemp("model_params") / "dense.npz")
        subprocess.check_call([sys.executable, "-m", "tests.step_plan_cases", path, which, ",".join(sets)], cwd=ROOT,
                              env=dict(os.environ, GRAAL_STRICT_DENSE="1"), timeout=600)
        out.update(np.load(path))
    return out


@pytest.mark.parametrize("name,params", FLOWS, ids=["%s-%s" % f for f in FLOWS])
def test_b_reference_arithmetic_flows_equal_the_dense_validation_kernel(name, params, dense_kernel):
    """Bit for bit (tests/test_step_plan_gpu.py); the anchored cases also within 2e-9 |logL| of the dense oracle run the reference's way
    (tests/test_strict_windowed_gpu.py)."""
    assert os.environ.get("GRAAL_STRICT_DENSE") in (None, "0")
    P, s, max_id = SC.layout_of(name, params)
    PC.assert_not_default(P["param_simu"])
    r = SC.run_case(name, params)
    got, want = r["deltas"], dense_kernel["d%d_%s" % (list(SC.CASES).index(name), params)]
    assert got.shape == want.shape
    PC.assert_reference_usable(np.nan_to_num(want), (name, params))
    bad = np.argwhere(got.view(np.int64) != want.view(np.int64))
    assert len(bad) == 0, (name, params, len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    assert r["moved"]["evaluations"] == len(SC.CASES[name]["props"]) and r["moved"]["fallbacks"] == 0, r["moved"]
    if name in ORACLE_ANCHORED:
        from graal_amd import synth
        from tests.test_repeats_gpu import oracle_deltas_with_repeats
        from tests.test_strict_gpu import ref_deltas
        from tests.test_strict_windowed_gpu import ref_dense
        repeats = bool(SC.CASES[name].get("repeats"))
        dense = ref_dense(P if "hic_matrix" in P else synth.with_dense(P))
        worst = 0.0
        for (fA, fBs), g in zip(SC.CASES[name]["props"], got):
            base, ref = (oracle_deltas_with_repeats if repeats else ref_deltas)(P, dense, s, fA, fBs, max_id)
            PC.assert_reference_usable(ref, (name, params, fA))
            err = np.abs(g - ref)
            worst = max(worst, report("b", "%s fA %d" % (name, fA), params, err, 2e-9 * abs(base)))
            assert np.all(err <= 2e-9 * abs(base)), (name, params, fA, fBs, err.max() / abs(base))


@pytest.mark.parametrize("params", PC.FITTED)
def test_b_exact_arithmetic_with_a_contig_above_1024_matches_the_dense_oracle(params):
    """1e-8 |logL| on grid coordinates (tests/test_step_plan_gpu.py, tests/test_engine_gpu.py)."""
    from tests.test_engine_gpu import dense_for, oracle_deltas
    r = SC.run_case(EXACT, params)
    assert r["facts"]["max_lcont"] == 1100 and r["moved"]["fallbacks"] == 0
    P, s, max_id = SC.layout_of(EXACT, params)
    PC.assert_not_default(P["param_simu"])
    dense = dense_for(P)
    for (fA, fBs), got in zip(SC.CASES[EXACT]["props"], r["deltas"]):
        base, want = oracle_deltas(P, dense, s, fA, fBs, max_id)
        PC.assert_reference_usable(want, (params, fA))
        err = np.abs(got - want)
        report("b", "exact arithmetic fA %d" % fA, params, err, 1e-8 * abs(base))
        assert err.max() <= 1e-8 * abs(base), (params, fA, fBs, err.max() / abs(base))


# ---- (c) the whole-layout scorers against their numpy restatements -------------------------------------------------------------------
SMALL = ("sub3", "sub1", "circ")
CUT_QUIRK = {"w1": False, "w3": True}                       # (tests/test_score_buffers_gpu.py's modes)
SMALL_SETS = [(n, q, p) for n in SMALL for q in (False, True) for p in PC.NAMES]
CUT_SETS = [(n, p) for n in ("w1", "w3") for p in PC.FITTED]


def small_case(name, params):
    return cached(("params-small", name, params), lambda: PC.with_params(JR.case(name), params))


def cut_case(name, params):
    def make():
        P = PC.with_params(WC.small_cut(name), params)
        assert P["param_simu"][PC.I_DMAX] == WC.small(name)["param_simu"][PC.I_DMAX]        # the case's own window
        return P
    return cached(("params-cut", name, params), make)


@pytest.mark.parametrize("name,quirk,params", SMALL_SETS)
def test_c_junction_scores_equal_the_restatement(name, quirk, params):
    """|q - J| <= 1e-9 A + 1 (tests/test_junctions_gpu.py)."""
    P = small_case(name, params)
    J, st_ref, A = JR.reference(P, quirk=quirk)
    PC.assert_no_status(st_ref, JUNCTION_NONFINITE, (name, params))
    ok_ref = st_ref == JUNCTION_VALID
    assert ok_ref.sum() >= 10
    PC.assert_fits_fixed_point(np.abs(J[ok_ref]) / Q, (name, params))
    e = engine_for(P, quirk=quirk)
    try:
        q, st = e.junction_scores_q()
    finally:
        e.close()
    assert np.array_equal(st, st_ref)
    ok = st == JUNCTION_VALID
    assert (q[~ok] == 0).all()
    report("c", "junctions %s quirk %d" % (name, quirk), params, np.abs(q[ok] - J[ok]), tol_q(A[ok]))
    assert np.all(np.abs(q[ok] - J[ok]) <= tol_q(A[ok])), np.max(np.abs(q[ok] - J[ok]))


@pytest.mark.parametrize("name,quirk,params", SMALL_SETS)
def test_c_ring_scores_equal_the_restatement(name, quirk, params):
    """|q - R| <= 1e-9 A + 1 (tests/test_rings_gpu.py); the scores do not read the mode flag."""
    P = small_case(name, params)
    R, Cn, St, A = cached(("params-rings", name, params), lambda: RR.ring_scores_windowed(P))[:4]
    PC.assert_no_status(St, RING_NONFINITE, (name, params))
    scored = St <= RING_OPEN
    assert (St == RING_CLOSE).sum() >= 10
    PC.assert_fits_fixed_point(np.abs(R[scored]) / Q, (name, params))
    e = engine_for(P, quirk=quirk)
    try:
        q, c, st = e.ring_scores_q()
    finally:
        e.close()
    assert np.array_equal(st, St) and np.array_equal(c, Cn) and (q[~scored] == 0).all()
    report("c", "rings %s quirk %d" % (name, quirk), params, np.abs(q[scored] - R[scored]), tol_q(A[scored]))
    assert np.all(np.abs(q[scored] - R[scored]) <= tol_q(A[scored])), float(np.max(np.abs(q[scored] - R[scored])))
    if name == "circ":
        assert (st[P["S_o_A_frags"]["circ"] == 1] == RING_OPEN).all()


@pytest.mark.parametrize("params", PC.FITTED)
def test_c_closing_rings_gains_the_difference_of_full_evaluations(params):
    """graal_close_rings committed on "circ": the summed scores equal eval_full(after) - eval_full(before) within the sum of 1e-9 A / 2^30 +
    (terms + 1) / 2^30, and the closed layout scores the opening as minus the closure, bit for bit (tests/test_rings_gpu.py)."""
    P = small_case("circ", params)
    s = P["S_o_A_frags"]
    parts = {}
    _, _, St, A = RR.ring_scores_windowed(P, parts=parts)[:4]
    PC.assert_no_status(St, RING_NONFINITE, params)
    e = engine_for(P)
    try:
        q, _, st = e.ring_scores_q()
        heads = [int(np.nonzero(s["id_c"] == c)[0][0]) for c in np.unique(s["id_c"]) if st[np.nonzero(s["id_c"] == c)[0][0]] == RING_CLOSE]
        assert len(heads) >= 1
        e.relabel_contigs()
        before = e.eval_full()
        e.close_rings(heads)
        e.relabel_contigs()
        after = e.eval_full()
        gain = sum(int(q[f]) for f in heads) / Q
        PC.assert_reference_usable([after - before, gain], params)
        tol = sum(1e-9 * A[f] / Q + (parts["terms"][f] + 1) / Q for f in heads)
        report("c", "close_rings circ", params, abs((after - before) - gain), tol)
        assert abs((after - before) - gain) <= tol, (after - before, gain, tol)
        q2, _, st2 = e.ring_scores_q()
        assert (st2[heads] == RING_OPEN).all() and np.array_equal(q2[heads], -q[heads])
    finally:
        e.close()


@pytest.mark.parametrize("name,params", CUT_SETS)
def test_c_end_links_equal_the_restatement(name, params):
    """Keys, contacts and statuses equal, |q - rq| <= 1e-9 A + 1 (tests/test_links_gpu.py); the best partners and the mutual-best links
    are those of the GPU's own table, ties included (tests/test_layout_scores_midsize_gpu.py)."""
    from graal_amd import links
    P, quirk = cut_case(name, params), CUT_QUIRK[name]
    s = P["S_o_A_frags"]
    for min_frags in (1, 3):
        ra, rb, rq, rc, rst, A = LR.restatement(P, quirk=quirk).links(s, min_frags)
        assert len(ra) >= 10 and (rst == LINK_VALID).all()
        PC.assert_fits_fixed_point(np.abs(rq) / Q, (name, params))
        e = engine_for(P, quirk=quirk)
        try:
            a, b, q, c, st = e.end_links_q(min_frags)
            be, bq, (ma, mb, mq) = e.end_links_best(min_frags)
        finally:
            e.close()
        assert np.array_equal(a, ra) and np.array_equal(b, rb) and np.array_equal(st, rst) and np.array_equal(c, rc)
        report("c", "links %s min_frags %d" % (name, min_frags), params, np.abs(q - rq), tol_q(A))
        assert np.all(np.abs(q - rq) <= tol_q(A)), np.max(np.abs(q - rq))
        t = links.table_from(s, a, b, c, np.where(st == LINK_VALID, q.astype(np.float64), np.nan))
        best = links.best_links(t, 1)
        want_e = np.full(2 * len(s["id_c"]), -1, dtype=np.int64)
        want_q = np.zeros(2 * len(s["id_c"]), dtype=np.int64)
        ends = 2 * best["frag"] + best["side"]
        want_e[ends] = 2 * best["partner_frag"] + best["partner_side"]
        want_q[ends] = best["score"].astype(np.int64)
        assert len(ends) >= 10
        assert np.array_equal(be, want_e) and np.array_equal(bq, want_q)
        m = links.mutual_best(t)
        assert np.array_equal(ma, 2 * m["frag_a"] + m["side_a"]) and np.array_equal(mb, 2 * m["frag_b"] + m["side_b"])
        assert np.array_equal(mq, m["score"].astype(np.int64))


@pytest.mark.parametrize("name,params", CUT_SETS)
def test_c_insertions_equal_the_restatement(name, params):
    """Keys, contacts and statuses equal, |q - rq| <= 1e-9 A + 1 (tests/test_insert_gpu.py)."""
    P, quirk = cut_case(name, params), CUT_QUIRK[name]
    s = P["S_o_A_frags"]
    max_frags = 4 if name == "w3" else 1
    rp, rf, rr, rq, rc, rst, A = IR.restatement(P, quirk=quirk).insertions(s, max_frags)
    assert len(rp) >= 20 and (rst == INSERT_VALID).all()
    PC.assert_fits_fixed_point(np.abs(rq) / Q, (name, params))
    e = engine_for(P, quirk=quirk)
    try:
        p, f, r, q, c, st = e.insertions_q(max_frags)
    finally:
        e.close()
    assert np.array_equal(p, rp) and np.array_equal(f, rf) and np.array_equal(r, rr)
    assert np.array_equal(st, rst) and np.array_equal(c, rc)
    report("c", "insertions %s max_frags %d" % (name, max_frags), params, np.abs(q - rq), tol_q(A))
    assert np.all(np.abs(q - rq) <= tol_q(A)), np.max(np.abs(q - rq))


def _spans_equal(family, name, params, sets, run, ref, valid, nonfinite):
    """The span scorers' comparison (tests/test_flips_gpu.py, test_swaps_gpu.py, test_excise_gpu.py): statuses and contacts equal,
    |q - rq| <= 1e-9 A + 1, at least 5 valid spans with contacts and a non-zero score."""
    want = [ref(*x) for x in sets]
    for rq, rc, rst, A in want:
        PC.assert_no_status(rst, nonfinite, (family, name, params))
    allq = np.concatenate([rq[rst == valid] for rq, rc, rst, A in want])
    PC.assert_fits_fixed_point(np.abs(allq) / Q, (family, name, params))
    P = cut_case(name, params)
    e = engine_for(P, quirk=CUT_QUIRK[name])
    try:
        got = [run(e, *x) for x in sets]
    finally:
        e.close()
    n_scored, errs, tols = 0, [], []
    for (q, c, st), (rq, rc, rst, A) in zip(got, want):
        assert np.array_equal(st, rst) and np.array_equal(c, rc)
        errs.append(np.abs(q - rq)); tols.append(tol_q(A))
        n_scored += int(((st == valid) & (q != 0) & (c > 0)).sum())
    err, tol = np.concatenate(errs), np.concatenate(tols)
    report("c", "%s %s" % (family, name), params, err, tol)
    assert np.all(err <= tol), float(np.max(err / tol))
    assert n_scored >= 5, n_scored


@pytest.mark.parametrize("name,params", CUT_SETS)
def test_c_block_flips_equal_the_restatement(name, params):
    P = cut_case(name, params)
    s = P["S_o_A_frags"]
    R = FR.restatement(P, quirk=CUT_QUIRK[name])
    _spans_equal("flips", name, params, list(flips.tilings(s, None, 4)), lambda e, first, last: e.block_flips_q(first, last),
                 lambda first, last: R.flips(s, first, last), FLIP_VALID, 3)


@pytest.mark.parametrize("name,params", CUT_SETS)
def test_c_block_swaps_equal_the_restatement(name, params):
    from tests.test_swaps_cpu import swap_sets
    P = cut_case(name, params)
    s = P["S_o_A_frags"]
    R = SR.restatement(P)
    _spans_equal("swaps", name, params, swap_sets(s), lambda e, first, mid, last: e.block_swaps_q(first, mid, last),
                 lambda first, mid, last: R.swaps(s, first, mid, last), SWAP_VALID, 2)


@pytest.mark.parametrize("name,params", CUT_SETS)
def test_c_block_excisions_equal_the_restatement(name, params):
    from tests.test_excise_cpu import long_runs
    P = cut_case(name, params)
    s = P["S_o_A_frags"]
    R = XR.restatement(P, quirk=CUT_QUIRK[name])
    _spans_equal("excisions", name, params, list(excise.tilings(s, None, 4)) + [long_runs(s)],
                 lambda e, first, last: e.block_excisions_q(first, last), lambda first, last: R.excisions(s, first, last), EXCISE_VALID, 3)


@pytest.mark.parametrize("name,params", CUT_SETS)
def test_c_layout_maps_equal_the_restatement(name, params):
    """layout_maps(64): order, binning and the observed image equal; |E - E_ref| <= 1e-6 E_ref + terms 2^-30 (tests/test_maps_gpu.py)."""
    P = cut_case(name, params)
    s = P["S_o_A_frags"]
    order, pix, b, m = MR.pixels(P["np_sub_frags_id"], s, 64)
    Ob = MR.observed(P["coo_row"], P["coo_col"], P["coo_val"], pix, m)
    a_, b_, lam = SIM.expected_lambda_matrix(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                                             P["mean_squared_frags_per_bin"], P["param_simu"], s)
    PC.assert_fits_fixed_point(lam, (name, params))
    Eref, N, _ = MR.expected_from_lambda(a_, b_, lam, pix, m)
    e = engine_for(P)
    try:
        Og, E, Rs, pixg, bg, bad = e.layout_maps(64)
    finally:
        e.close()
    assert bg == b and Og.shape == E.shape == Rs.shape == (m, m) and np.array_equal(pixg, pix)
    assert np.array_equal(Og, Ob) and Ob.sum() > 0 and bad == 0
    err = np.abs(E.astype(np.float64) - Eref)
    tol = 1e-6 * Eref + N * 2.0 ** -30
    report("c", "maps64 %s" % name, params, err.ravel(), np.maximum(tol, 1e-300).ravel())
    assert np.all(err <= tol), float(np.max(err / np.maximum(tol, 1e-300)))
    assert np.array_equal(E, E.T) and np.all(E >= 0)
    r, want = Rs.astype(np.float64), MR.residual(Og.astype(np.float64), E.astype(np.float64))
    rtol = 2.0 ** -22 * ((np.abs(Og) + np.abs(E)) / np.sqrt(np.where(E > 0, E, 1.0)) + np.abs(want)) + 1e-30
    assert np.all(np.abs(r - want) <= rtol)


@pytest.mark.parametrize("params", PC.FITTED)
def test_c_simulated_contacts_equal_the_restatement(params):
    """tests/test_simulate_gpu.py's smallest problem (a ring, RF counts 9, 240 sub-fragments): the draws equal sim_reference's but for the
    flagged last-place roundings, at most ceil(1e-4 nnz) of them."""
    from graal_amd.simulate import simulate_contacts
    from tests.test_simulate_gpu import _case, _well_formed
    P, _ = _case("circ")
    P = PC.with_params(P, params)
    par = P["param_simu"]
    a_, b_, lam = SIM.expected_lambda_matrix(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                                             P["mean_squared_frags_per_bin"], par, P["S_o_A_frags"])
    PC.assert_fits_fixed_point(lam, params)
    want = SIM.simulate(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"], par,
                        P["S_o_A_frags"], 77)
    nnz = len(want[0])
    assert nnz > 500
    got = simulate_contacts(P, 77)
    diff, unexplained = SIM.compare(got, want[:3], want[3], want[4])
    print("\n[params] c | simulate circ | %s: %d of %d entries differ (all flagged), allowed %d" % (params, len(diff), nnz, math.ceil(1e-4 * nnz)))
    assert unexplained == [], unexplained[:10]
    assert len(diff) <= math.ceil(1e-4 * nnz), (len(diff), nnz)
    _well_formed(*got, P["init_n_sub_frags"])


# ---- (d) the own-pixel carry ---------------------------------------------------------------------------------------------------------
def test_d_carried_total_plus_the_commits_own_pixels_is_the_full_likelihood(monkeypatch):
    """150 steps from three contigs, two of them rings, under fitted_a, checked every 7 steps at tests/test_carried_total_gpu.py's REL."""
    from tests import test_carried_total_gpu as CT
    P = CT.close_into_circles(PC.with_params(CT.problem(), "fitted_a"), (1, 3))
    PC.assert_not_default(P["param_simu"])
    a = CT.run(P, 5, 150, 7, monkeypatch)
    assert a["own"] and a["circ"] > 0
    assert a["corr"] > 1e-6, "no commit changed an own pixel: the test did not test anything"
    assert a["counters"]["carried_totals_repaired"] == 0
    print("\n[params] d | carried total | fitted_a: worst |carried - full| / tolerance = %.3g, largest correction %.3e" % (a["worst"] / CT.REL, a["corr"]))
    assert a["worst"] <= CT.REL


def test_d_carried_run_under_fitted_parameters_against_the_oracle():
    """The test above holds the carried total to the engine's own full evaluation, which a wrong model passes; this one anchors the same
    problem outside the engine (tests/test_carried_total_gpu.py::test_carried_run_against_the_oracle, its tolerances): one cycle of
    start_EM, 90 steps, against the oracle run the reference's way -- accepted moves and layout bit for bit, the likelihood series to 1e-8."""
    from tests import test_carried_total_gpu as CT
    from tests.test_strict_gpu import _run, _samplers
    P = CT.close_into_circles(PC.with_params(CT.problem(), "fitted_a"), (1, 3))
    ora, g, gpu_rng = _samplers(P, 9, "strict")
    assert g._own_corr
    t_ref = _run(ora, ora.rng, 4, 90, scrambled=False)
    PC.assert_reference_usable(t_ref.likelihood, "fitted_a")
    assert len(t_ref.likelihood) == 90 and len(np.unique(np.asarray(t_ref.mutations())[:, 2])) >= 3
    t_gpu = _run(g, gpu_rng, 4, 90, scrambled=False)
    assert np.array_equal(t_gpu.mutations(), t_ref.mutations())
    got, want = np.asarray(t_gpu.likelihood, np.float64), np.asarray(t_ref.likelihood, np.float64)
    report("d", "carried run vs oracle", "fitted_a", np.abs(got - want), 1e-8 * np.abs(want))
    assert np.allclose(got, want, rtol=1e-8, atol=0)
    g.gpu_vect_frags.copy_from_gpu()
    for k in O.FIELDS:
        assert np.array_equal(getattr(g.gpu_vect_frags, k), ora.gpu_vect_frags[k]), k
    assert g.engine.run_counters()["carried_totals_repaired"] == 0
    g.free_gpu()


# ---- (e) a parameter change on a used handle -----------------------------------------------------------------------------------------
def _used_handle_calls():
    from tests.test_score_buffers_gpu import CALLS, flat
    P0 = WC.small_cut("w3")
    s = P0["S_o_A_frags"]
    lists = LR.contigs_of(s)
    long_ = sorted((m for m in lists.values() if len(m) >= 25), key=len)
    short = sorted((m for m in lists.values() if len(m) <= 4), key=len)
    assert len(long_) >= 2 and len(short) >= 2
    props = [(int(long_[0][3]), [int(long_[1][5]), int(short[0][0]), int(long_[0][10])]),
             (int(short[1][0]), [int(long_[-1][0]), int(long_[-1][-1]), int(short[0][0])])]

    # every call relabels first (idempotent): the used handle and the fresh ones hold the same labels whatever ran before
    def candidates(strict, i):
        def call(e):
            e.set_mode(ref_trans_accu=strict, strict=strict)                # (reference arithmetic with, exact arithmetic without the quirk)
            max_id = e.relabel_contigs()
            out = np.array(e.eval_candidates(props[i][0], np.asarray(props[i][1], np.int32), max_id))
            e.set_mode(ref_trans_accu=True, strict=False)
            return (out,)
        return call

    def full(e):
        e.relabel_contigs()
        return (np.array(e.eval_full_q()),)

    def scorer(fn):
        def call(e):
            e.relabel_contigs()
            return fn(e)
        return call

    calls = {"full": full}
    for strict in (True, False):
        for i in range(2):
            calls["candidates-%s-%d" % ("strict" if strict else "exact", i)] = candidates(strict, i)
    calls.update({k: scorer(fn) for k, fn in CALLS.items()})
    return P0, calls, flat


def test_e_parameter_changes_on_a_used_handle_equal_fresh_handles():
    """default -> fitted_a -> fitted_b at d_max 4 kb -> fitted_a at d_max 40 kb -> default on ONE engine (small_cut("w3"), the quirk on):
    behind every change the full evaluation, two candidate evaluations in each arithmetic and every call of
    tests/test_score_buffers_gpu.CALLS equal, as arrays of equal dtype, the same call made first on a fresh handle created with those
    parameters; re-sending the set in force changes nothing."""
    P0, calls, flat = _used_handle_calls()
    own = np.asarray(P0["param_simu"], np.float32)
    sequence = [("default", own), ("fitted_a", PC.param("fitted_a", own)), ("fitted_b-4kb", PC.param("fitted_b", own, d_max=4.0)),
                ("fitted_a-40kb", PC.param("fitted_a", own, d_max=40.0)), ("default", own)]
    dmax = [float(p[PC.I_DMAX]) for _, p in sequence]
    assert dmax[2] < min(dmax[:2]) and dmax[3] > max(dmax[:3]), dmax       # shrinks below, then grows beyond, everything so far
    fresh = {}

    def fresh_result(label, par, call):
        if (label, call) not in fresh:
            f = engine_for(dict(P0, param_simu=par), quirk=True)
            try:
                fresh[label, call] = flat(calls[call](f))
            finally:
                f.close()
        return fresh[label, call]

    e = engine_for(P0, quirk=True)
    try:
        seen = {}
        for step, (label, par) in enumerate(sequence):
            e.set_params(par)
            assert np.array_equal(e.param, par)
            for call in calls:
                got, want = flat(calls[call](e)), fresh_result(label, par, call)
                assert len(got) == len(want)
                for i, (g, w) in enumerate(zip(got, want)):
                    assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (step, label, call, i)
            full_before = flat(calls["full"](e))
            e.set_params(par)                                                # (the set in force, sent again)
            for call in ("full", "candidates-strict-0", "links1", "rings"):
                for g, w in zip(flat(calls[call](e)), fresh_result(label, par, call)):
                    assert np.array_equal(g, w, equal_nan=g.dtype.kind == "f"), (step, label, call)
            assert np.array_equal(flat(calls["full"](e))[0], full_before[0])
            seen[label] = fresh_result(label, par, "full")[0]
        # the sets are told apart: no two of them give the same full evaluation, candidates or ring scores
        labels = list(seen)
        for call in ("full", "candidates-strict-0", "candidates-exact-1", "rings", "links1"):
            for i in range(len(labels)):
                for j in range(i):
                    a, b = fresh[labels[i], call], fresh[labels[j], call]
                    assert any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b)), (call, labels[i], labels[j])
    finally:
        e.close()


# ---- (f) the sampler -----------------------------------------------------------------------------------------------------------------
def test_f_trace_with_nuisance_parameter_sampling_from_a_fitted_start_matches_the_oracle():
    """tests/test_sampler_gpu.py::test_trace_with_nuisance_parameter_sampling_matches_oracle from a start at fitted_a: accepted moves, the
    success series and the walk of (fact, slope, d_max, v_inter) bit for bit, the likelihood series at rtol 1e-8."""
    from tests.test_sampler_gpu import make_gpu_sampler, problem
    P = PC.with_params(problem(3, 46, 45, 900), "fitted_a")
    PC.assert_not_default(P["param_simu"])
    P["bins"] = np.arange(2.0, 60.0, 2.0)
    ora = O.OracleSampler(P, np.random.RandomState(46), fix_trans_accu=True)
    t_ref = em.run_em(ora, 1, 3, rng=ora.rng, sample_param=True)
    PC.assert_reference_usable(t_ref.likelihood_nuisance, "fitted_a")
    gpu_rng = np.random.RandomState(46)
    g = make_gpu_sampler(P, gpu_rng)
    g.bins = P["bins"]
    t_gpu = em.run_em(g, 1, 3, rng=gpu_rng, sample_param=True)
    assert np.array_equal(t_gpu.mutations(), t_ref.mutations())
    assert t_gpu.success == t_ref.success and 0 < sum(t_ref.success) < len(t_ref.success)
    for a, b in ((t_gpu.fact, t_ref.fact), (t_gpu.slope, t_ref.slope), (t_gpu.d_max, t_ref.d_max), (t_gpu.d_nuc, t_ref.d_nuc)):
        assert np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32))
    assert np.float32(t_ref.slope[0]) != np.float32(-1.5) and len(set(np.asarray(t_ref.slope, np.float32).tolist())) > 1
    got, want = np.asarray(t_gpu.likelihood_nuisance, np.float64), np.asarray(t_ref.likelihood_nuisance, np.float64)
    report("f", "nuisance likelihood series", "fitted_a", np.abs(got - want), 1e-8 * np.abs(want))
    assert np.allclose(got, want, rtol=1e-8, atol=0)
    g.gpu_vect_frags.copy_from_gpu()
    for k in O.FIELDS:
        assert np.array_equal(getattr(g.gpu_vect_frags, k), ora.gpu_vect_frags[k]), k
    g.free_gpu()


# ---- (g) refusals --------------------------------------------------------------------------------------------------------------------
FIELDS = {"kuhn": PC.I_KUHN, "lm": PC.I_LM, "c1": PC.I_C1, "slope": PC.I_SLOPE, "d": PC.I_D, "fact": PC.I_FACT}
REFUSED = [(f, v) for f in FIELDS for v in (np.nan, np.inf, -np.inf)] + [("kuhn", 0.0), ("kuhn", -1.0), ("lm", 0.0), ("lm", -9.6)]


@pytest.mark.parametrize("params", [None, "fitted_a"])
def test_g_set_params_refuses_what_the_model_cannot_price(params):
    """A non-finite kuhn, lm, c1, slope, d or fact, and kuhn <= 0 or lm <= 0: GRAAL_E_ARG with a message that names the field; the
    parameters in force, the host copy of them and the full evaluation are what they were."""
    P = JR.case("sub3") if params is None else small_case("sub3", params)
    good = np.asarray(P["param_simu"], np.float32)
    e = engine_for(P)
    try:
        e.relabel_contigs()
        before = np.array(e.eval_full_q())
        assert before.any()
        for field, value in REFUSED:
            bad = good.copy()
            bad[FIELDS[field]] = value
            with pytest.raises(GraalError, match=r"graal_set_params: %s must .*\(code 1\)" % field):
                e.set_params(bad)
            assert np.array_equal(e.param, good), (field, value)
            assert np.array_equal(np.array(e.eval_full_q()), before), (field, value)
        e.set_params(good)                                                   # (the set in force: accepted, nothing moves)
        assert np.array_equal(np.array(e.eval_full_q()), before)
        other = PC.param("fitted_b", good)                                   # and a valid change still takes effect behind the refusals
        e.set_params(other)
        assert not np.array_equal(np.array(e.eval_full_q()), before)
    finally:
        e.close()
    # a fresh handle refuses them as its first parameters too, and then has none
    from graal_amd.lib import Engine
    f = Engine(0)
    try:
        bad = good.copy()
        bad[PC.I_SLOPE] = np.nan
        with pytest.raises(GraalError, match="slope"):
            f.set_params(bad)
        assert not hasattr(f, "param")
        with pytest.raises(GraalError):
            f.eval_full()
    finally:
        f.close()
