"""graal_junction_gaps at a mid-size shape: tests/window_cases.m2 (contigs of 500 .. 1,100 bins, each longer than the contact window;
n_sub 3, mixed RF counts, reversed bins) without its last contact, on a fresh engine and on a stepped one, five gap values, against
the vectorised restatement (tests/junction_gap_reference.py on tests/window_reference.py).  The list is row-sorted, 119,999 contacts:
its last wave is short and rows' contacts span two waves; contigs above 1,024 bins take several stripes of the mass kernel once the
engine has stepped."""
import numpy as np
import pytest

from graal_amd.lib import JUNCTION_VALID
from tests import junction_boot_reference as BR
from tests import junction_gap_reference as GR
from tests.engine_states import engine_in

pytestmark = pytest.mark.gpu
_REF = {}


def tol(A):
    return 1e-9 * np.asarray(A, np.float64) + 1           # tests/test_layout_scores_midsize_gpu.py's bound, in Q


def mid_grid(P):
    """0, a value below a bin's length, two that carry some of the window's pairs across d_max, and d_max itself."""
    d_max = np.float32(P["param_simu"][5])
    return np.array([0.0, 0.3, 0.05 * d_max, 0.4 * d_max, d_max], np.float32)


def restatement(P):
    if "m2" not in _REF:
        _REF["m2"] = GR.vectorised(P, mid_grid(P))
    return _REF["m2"]


@pytest.mark.parametrize("quirk", [False, True])
def test_profile_equals_restatement_fresh_and_stepped(quirk):
    P = BR.mid_case()
    row = np.asarray(P["coo_row"])
    assert len(row) == 119_999 and (np.diff(row) >= 0).all()
    ends = np.arange(63, len(row) - 1, 64)                 # a wave's last contact and the next wave's first one in the same row
    assert (row[ends] == row[ends + 1]).sum() >= 100
    grid = mid_grid(P)
    G, st, A = restatement(P)                              # (the pairs stay cis: one restatement serves both modes)
    got = {}
    for engine_state in ("fresh", "stepped"):
        e, s, Sw = engine_in(engine_state, P, quirk=quirk)
        try:
            scores = e.junction_scores_q()
            g = e.junction_gaps_q(grid, GR.DROP_Q, profile=True)
        finally:
            e.close()
        got[engine_state] = g
        assert Sw == (3 if engine_state == "stepped" else 1)
        assert (s["l_cont"] > 1024).any()
        # (a profile does not depend on its contig's label: one restatement, of the problem's own layout, serves both engines)
        s0 = P["S_o_A_frags"]
        assert all(np.array_equal(s[k], s0[k]) for k in s0 if k != "id_c")
        assert np.array_equal(g["q"], scores[0]) and np.array_equal(g["status"], scores[1])
        assert np.array_equal(g["status"], st)
        ok = g["status"] == JUNCTION_VALID
        assert ok.sum() >= 2990
        prof = g["q_gap"]
        assert prof.shape == G.shape == (5, len(st)) and not prof[:, ~ok].any() and not prof[0].any()
        excess = np.abs(prof - G)[:, ok] / tol(A[:, ok])
        print("m2 quirk %d %s: %d cells, largest |q_gap - G| / tolerance %.3e" % (quirk, engine_state, excess.size, float(excess.max())))
        assert (excess <= 1).all(), int((excess > 1).sum())
        assert (prof[1:, ok] != 0).all()
        if not quirk:
            assert (np.abs(prof[4] + g["q"])[ok] <= tol(A[4][ok])).all()     # a gap of d_max is a cut
        for k, w in zip(("best", "q_best", "lo", "hi"), GR.fold(prof, g["status"], GR.DROP_Q)):
            assert np.array_equal(g[k], w), k
    for k in got["fresh"]:
        assert np.array_equal(got["fresh"][k], got["stepped"][k]), k
