"""CPU: the restatements of graal_ring_scores and graal_close_rings (tests/ring_reference.py) -- the vectorised one equal to the brute-force
one, both equal to the difference of two full re-scores, the commit's rules, the planner, and the signal on simulated data."""
import numpy as np
import pytest

from graal_amd import rings
from graal_amd.lib import RING_CLOSE, RING_NONFINITE, RING_OPEN, RING_SINGLE
from oracle.sparse_numpy import SparseScorer
from tests import edit_reference as ER
from tests import junction_reference as JR
from tests import ring_reference as RR
from tests import sim_reference as SR
from tests import window_cases as WC
from tests.engine_states import cached
from tests.util import check_invariants

Q = float(1 << 30)
CASES = ("sub3", "sub1", "circ", "w1", "w3")


def problem(name):
    if name in ("w1", "w3"):
        return cached(("rings", name), lambda: RR.with_rings(WC.small_cut(name), 2))
    return cached(("rings", name), lambda: JR.case(name))


def brute(name):
    def run():
        parts = {}
        return RR.ring_scores(problem(name), parts=parts) + (parts,)
    return cached(("rings-brute", name), run)


def contigs_of(s):
    return [(int(c), np.nonzero(s["id_c"] == c)[0]) for c in np.unique(s["id_c"])]


def test_status_constants_agree():
    assert (RR.CLOSE, RR.OPEN, RR.SINGLE, RR.NONFINITE) == (RING_CLOSE, RING_OPEN, RING_SINGLE, RING_NONFINITE)
    from graal_amd import lib
    assert (RR.EDIT_OK, RR.EDIT_BAD_FRAG, RR.EDIT_CIRCULAR, RR.EDIT_SINGLE, RR.EDIT_TWICE) == \
        (lib.RINGEDIT_OK, lib.RINGEDIT_BAD_FRAG, lib.RINGEDIT_CIRCULAR, lib.RINGEDIT_SINGLE, lib.RINGEDIT_TWICE)


@pytest.mark.parametrize("name", CASES)
def test_windowed_equals_brute_force(name):
    P = problem(name)
    R, C, St, A, parts = brute(name)
    wp = {}
    R2, C2, St2, A2 = RR.ring_scores_windowed(P, parts=wp)
    assert np.array_equal(St, St2) and np.array_equal(C, C2)
    assert np.array_equal(R, R2) and np.array_equal(A, A2)
    for k in ("terms", "contact", "mass", "own"):
        assert np.array_equal(parts[k], wp[k]), k
    s = P["S_o_A_frags"]
    assert (St == RING_CLOSE).any() and np.all(St[(s["circ"] != 1) & (s["l_cont"] < 2)] == RING_SINGLE)
    if name in ("circ", "w1", "w3"):
        assert ((St == RING_OPEN) | (St == RING_NONFINITE))[s["circ"] == 1].all() and (s["circ"] == 1).any()
    assert np.abs(parts["contact"]).max() > 0 and np.abs(parts["mass"]).max() > 0
    if name in ("sub3", "circ", "w3"):
        assert np.abs(parts["own"]).max() > 0


@pytest.mark.parametrize("name", CASES)
def test_equals_the_difference_of_two_full_rescores(name):
    """R / 2^30 = full(toggled) - full(current) within 1e-9 A / 2^30 + 2^-30 (terms + 1): the junction tests' tolerance plus one Q
    rounding per contact and fragment pair inside the window."""
    P = problem(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    R, C, St, A, parts = brute(name)
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    base = sp.full(s)
    checked = 0
    for c, m in contigs_of(s):
        f = int(m[0])
        if St[f] not in (RING_CLOSE, RING_OPEN) or len(m) < 2:
            continue
        want = sp.full(RR.toggle(s, c)) - base
        tol = 1e-9 * A[f] / Q + (parts["terms"][f] + 1) / Q
        print(name, c, len(m), R[f] / Q, want, abs(R[f] / Q - want), tol)
        assert abs(R[f] / Q - want) <= tol, (c, R[f] / Q, want, tol)
        checked += 1
    assert checked >= 2


def test_open_is_minus_close_bit_for_bit():
    P = problem("circ")
    s = P["S_o_A_frags"]
    R, _, St, _, _ = brute("circ")
    t = s
    for c, _ in contigs_of(s):
        t = RR.toggle(t, c)
    R2, _, St2, _ = RR.ring_scores_windowed(P, t)
    ok = (St <= RING_OPEN) & (St2 <= RING_OPEN)
    assert ok.all() and np.array_equal(R2, -R) and np.array_equal(St2, 1 - St)


def test_close_rules_and_refusals():
    P = problem("w1")
    s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
    linear = [m for _, m in contigs_of(s) if s["circ"][m[0]] != 1 and len(m) >= 2]
    ring = next(m for _, m in contigs_of(s) if s["circ"][m[0]] == 1)
    single = next(m for _, m in contigs_of(s) if s["circ"][m[0]] != 1 and len(m) == 1)
    assert len(linear) >= 3
    frags = [int(linear[0][0]), int(linear[1][len(linear[1]) // 2]), int(linear[2][-1])]
    out, st = RR.close(s, frags)
    assert (st == RR.EDIT_OK).all()
    check_invariants(out)
    for k in s:
        if k not in ("circ", "prev", "next"):
            assert np.array_equal(out[k], s[k]), k
    changed = np.concatenate(linear[:3])
    rest = np.setdiff1d(np.arange(len(s["pos"])), changed)
    for k in ("circ", "prev", "next"):
        assert np.array_equal(out[k][rest], s[k][rest]), k
    assert (out["circ"][changed] == 1).all()
    # cutting a closed contig after its last-position fragment gives the original back, field for field
    cuts = [int(m[np.argmax(s["pos"][m])]) for m in linear[:3]]
    back, st = ER.edit(out, cuts=cuts)
    assert back is not None and (st == 0).all()
    for k in s:
        assert np.array_equal(back[k], s[k]), k
    # every refusal once
    n = len(s["pos"])
    for bad, code in (([n], RR.EDIT_BAD_FRAG), ([-1], RR.EDIT_BAD_FRAG), ([int(ring[0])], RR.EDIT_CIRCULAR), ([int(single[0])], RR.EDIT_SINGLE)):
        out, st = RR.close(s, [frags[0]] + bad)
        assert out is None and list(st) == [RR.EDIT_OK, code]
    out, st = RR.close(s, [int(linear[0][0]), frags[1], int(linear[0][-1])])
    assert out is None and list(st) == [RR.EDIT_TWICE, RR.EDIT_OK, RR.EDIT_TWICE]


def test_plan_rings():
    table = {"score": np.array([5.0, -1.0, 0.5, np.nan, 3.0, np.nan, -2.0, 0.0]),
             "status": np.array([RING_CLOSE, RING_CLOSE, RING_CLOSE, RING_SINGLE, RING_OPEN, RING_NONFINITE, RING_OPEN, RING_CLOSE], np.uint8)}
    assert list(rings.plan_rings(table)) == [0, 2]
    assert list(rings.plan_rings(table, min_score=1.0)) == [0]
    assert list(rings.plan_rings(table, open_rings=True)) == [0, 2, 4]
    assert list(rings.plan_rings(table, min_score=4.0, open_rings=True)) == [0]
    assert list(rings.plan_rings(table, min_score=-5.0)) == [0, 1, 2, 7]
    assert list(rings.plan_rings({"score": np.zeros(0), "status": np.zeros(0, np.uint8)})) == []


TRUTHS = ("as_is", "linear", "rings")


def truth_layout(which):
    P = problem("circ")
    s = P["S_o_A_frags"]
    for c, m in contigs_of(s):
        ring = s["circ"][m[0]] == 1
        if (which == "linear" and ring) or (which == "rings" and not ring):
            s = RR.toggle(s, c)
    return s


def simulated(which, seed):
    def run():
        P = dict(problem("circ"))
        s = truth_layout(which)
        r, c, v = SR.simulate(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
                              P["param_simu"], s, seed)[:3]
        P["coo_row"], P["coo_col"], P["coo_val"] = np.asarray(r), np.asarray(c), np.asarray(v)
        P["S_o_A_frags"] = s
        return P
    return cached(("rings-sim", which, seed), run)


@pytest.mark.parametrize("which", TRUTHS)
@pytest.mark.parametrize("seed", (7, 8, 9))
def test_truth_is_recovered(which, seed):
    """Every toggle of a true topology scores below 0; so in the truth with its rings opened, exactly the true rings score above 0."""
    P = simulated(which, seed)
    s = P["S_o_A_frags"]
    R, _, St, _ = RR.ring_scores_windowed(P)
    heads = [int(m[0]) for _, m in contigs_of(s)]
    print(which, seed, [(int(St[f]), R[f] / Q) for f in heads])
    assert len(heads) == 2 and all(St[f] in (RING_CLOSE, RING_OPEN) for f in heads)
    assert all(R[f] < 0 for f in heads)
    opened = s
    for c, m in contigs_of(s):
        if s["circ"][m[0]] == 1:
            opened = RR.toggle(opened, c)
    R2, _, St2, _ = RR.ring_scores_windowed(P, opened)
    table = {"score": R2[heads] / Q, "status": St2[heads]}
    assert (St2[heads] == RING_CLOSE).all()
    assert [heads[i] for i in rings.plan_rings(table)] == [f for f in heads if s["circ"][f] == 1]
