"""The windowed restatement (tests/window_reference.py) pinned to the brute-force ones (tests/junction_reference.py, link_reference.py,
insert_reference.py): keys, statuses, contact counts, Q and the sums of |terms| equal as integers -- on the GPU tests' small problems
with their parameters, and on two problems whose contigs are several contact windows long (tests/window_cases.small)."""
import numpy as np
import pytest

from tests import insert_reference as IR
from tests import junction_reference as JR
from tests import link_reference as LR
from tests import window_cases as WC
from tests import window_reference as WR

_CASES = {}


def case(kind, name):
    if (kind, name) not in _CASES:
        if kind == "junction":
            _CASES[kind, name] = JR.case(name) if name in ("sub3", "sub1", "circ") else WC.small(name)
        else:
            _CASES[kind, name] = LR.case(name) if name in ("sub3", "sub1", "circ") else WC.small_cut(name)
    return _CASES[kind, name]


def _equal(ref, got):
    assert len(ref) == len(got)
    for k, (x, y) in enumerate(zip(ref, got)):
        assert np.array_equal(np.asarray(x, np.int64), np.asarray(y, np.int64)), (k, np.nonzero(np.asarray(x) != np.asarray(y))[0][:5])


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("sub1", True), ("circ", False), ("circ", True),
                                        ("w1", False), ("w3", False), ("w3", True)])
def test_junctions_equal_brute_force(name, quirk):
    P = case("junction", name)
    ref = JR.reference(P, quirk=quirk)
    got = WR.window(P, quirk).junction_scores(P["S_o_A_frags"])
    _equal(ref, got)
    assert (got[1] == WR.J_VALID).sum() >= 10


@pytest.mark.parametrize("name,quirk,min_frags", [("sub3", False, 1), ("sub3", True, 1), ("sub3", True, 3), ("sub1", False, 1),
                                                  ("sub1", False, 4), ("sub1", True, 4), ("circ", False, 1), ("circ", True, 2),
                                                  ("w1", False, 1), ("w3", True, 1), ("w3", False, 3)])
def test_links_equal_brute_force(name, quirk, min_frags):
    P = case("link", name)
    s = P["S_o_A_frags"]
    ref = LR.restatement(P, quirk=quirk).links(s, min_frags)
    got = WR.window(P, quirk).links(s, min_frags)
    _equal(ref, got)
    assert len(got[0]) >= 10


@pytest.mark.parametrize("name,quirk,max_frags", [("sub3", False, 1), ("sub3", True, 4), ("sub3", False, 4), ("sub1", False, 4),
                                                  ("sub1", True, 1), ("circ", True, 4), ("w1", False, 1), ("w3", True, 4),
                                                  ("w3", False, 1)])
def test_insertions_equal_brute_force(name, quirk, max_frags):
    P = case("link", name)
    s = P["S_o_A_frags"]
    ref = IR.restatement(P, quirk=quirk).insertions(s, max_frags)
    got = WR.window(P, quirk).insertions(s, max_frags)
    _equal(ref, got)
    assert len(got[0]) >= 10


@pytest.mark.parametrize("name", ["w1", "w3"])
def test_small_cases_reach_past_the_window(name):
    """Contigs several windows long, and cut pieces longer than the window: pairs beyond it exist and the restatement leaves them out."""
    P = case("junction", name)
    s = P["S_o_A_frags"]
    reach = WR.reach_bp(P["param_simu"][5])
    assert (s["l_cont_bp"] > 3 * reach).all()
    cut = case("link", name)["S_o_A_frags"]
    sizes = np.bincount(cut["id_c"])
    assert (np.bincount(cut["id_c"], weights=cut["len_bp"])[sizes >= 25] > reach).all() and ((sizes >= 1) & (sizes <= 4)).sum() >= 8


@pytest.mark.parametrize("name,quirk", [("w3", True), ("w1", False)])
def test_prefix_sums_equal_direct_sums(name, quirk):
    """Every junction's prefix-sum score equals its direct sum over the pairs and contacts that straddle it; the term classes add up."""
    P = case("junction", name)
    s = P["S_o_A_frags"]
    W = WR.window(P, quirk)
    parts = {}
    J, st, A = W.junction_scores(s, parts)
    frags = np.nonzero(st != WR.J_END)[0]
    frags = frags[s["circ"][frags] == 0]
    direct = W.junction_direct(s, frags)
    for f in frags:
        j, bad, a = direct[int(f)]
        assert (j, bad, a) == (J[f], st[f] == WR.J_NONFINITE, A[f]), f
    ok = st == WR.J_VALID
    assert np.array_equal(sum(parts.values())[ok], J[ok])
    assert (np.abs(parts["near"]) > 1e-9 * A + 1).sum() >= 3 and (np.abs(parts["contacts"]) > 1e-9 * A + 1).sum() >= 3
    if quirk:
        assert (np.abs(parts["far"]) > 1e-9 * A + 1).sum() >= 3


def test_link_and_insertion_parts_add_up():
    P = case("link", "w3")
    s = P["S_o_A_frags"]
    W = WR.window(P, True)
    a, b, c = W.link_keys(s)
    parts = []
    q, st, A = W.link_scores(s, a, b, parts)
    for k in ("contacts", "mass", "far", "mirror"):
        assert sum(abs(p.get(k, 0)) > 1e-9 * x + 1 for p, x in zip(parts, A)) >= 3, k
    assert all(sum(p.values()) == x for p, x in zip(parts, q))
    p, f, r, c = W.insertion_keys(s, 4)
    parts = []
    q, st, A = W.insertion_scores(s, p, f, r, parts)
    for k in ("contacts", "contacts_t12", "mass", "t12", "far", "mirror"):
        assert sum(abs(x.get(k, 0)) > 1e-9 * y + 1 for x, y in zip(parts, A)) >= 3, k
    assert all(sum(x.values()) == y for x, y in zip(parts, q))
