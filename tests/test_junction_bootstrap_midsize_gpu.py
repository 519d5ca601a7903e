"""graal_junction_bootstrap at a mid-size shape: tests/window_cases.m2 (contigs of 500 .. 1,100 bins, each longer than the contact window;
n_sub 3, mixed RF counts, reversed bins) without its last contact, on a fresh engine and on a stepped one, four replicates, against the
vectorised restatement (tests/junction_boot_reference.py on tests/window_reference.py).  The list is row-sorted, 119,999 contacts: its
last wave is short, and rows' contacts span two waves, so the run sums across a wave and the tails at its ends carry most rows."""
import numpy as np
import pytest

from graal_amd.lib import JUNCTION_VALID
from tests import junction_boot_reference as BR
from tests.engine_states import engine_in

pytestmark = pytest.mark.gpu


def tol(A):
    return 1e-9 * np.asarray(A, np.float64) + 1           # tests/test_layout_scores_midsize_gpu.py's bound, in Q


@pytest.mark.parametrize("quirk", [False, True])
def test_replicates_equal_restatement_fresh_and_stepped(quirk):
    P = BR.mid_case()
    row = np.asarray(P["coo_row"])
    assert len(row) % 64 != 0 and (np.diff(row) >= 0).all()
    ends = np.arange(63, len(row) - 1, 64)                 # a wave's last contact and the next wave's first one in the same row
    assert (row[ends] == row[ends + 1]).sum() >= 100
    got = {}
    for engine_state in ("fresh", "stepped"):
        e, s, Sw = engine_in(engine_state, P, quirk=quirk)
        try:
            scores = e.junction_scores_q()
            g = e.junction_bootstrap_q(BR.MID_SEED, BR.MID_REPS, 0, replicates=True)
        finally:
            e.close()
        got[engine_state] = g
        assert Sw == (3 if engine_state == "stepped" else 1)
        assert (s["l_cont"] > 1024).any()
        # (a junction's score does not depend on its contig's label: one restatement, of the problem's own layout, serves both engines)
        s0 = P["S_o_A_frags"]
        assert all(np.array_equal(s[k], s0[k]) for k in s0 if k != "id_c")
        pairs = np.unique(np.asarray(s0["id_c"], np.int64) * (len(row) + 1) + s["id_c"])
        assert len(pairs) == len(np.unique(s0["id_c"])) == len(np.unique(s["id_c"]))
        B, (J, A, flagged, nf) = BR.mid_replicates(quirk)
        assert (s["l_cont_bp"] > B.W.reach).all()          # every contig leaves the window: contacts without a term
        assert len(B.k) < len(row) - 1000
        # the data's own scores, word for word
        assert np.array_equal(g["q"], scores[0]) and np.array_equal(g["status"], scores[1])
        assert np.array_equal(g["status"], B.status) and not nf.any()
        ok = g["status"] == JUNCTION_VALID
        assert ok.sum() >= 2990
        # the replicates
        rep = g["q_rep"]
        assert rep.shape == J.shape and not rep[:, ~ok].any()
        cells = ok[None, :] & ~flagged
        assert cells.sum() >= 0.98 * ok.sum() * BR.MID_REPS
        excess = np.abs(rep - J)[cells] / tol(A[cells])
        print("m2 quirk %d %s: %d cells, %d flagged, largest |q_rep - J*| / tolerance %.3e" % (quirk, engine_state, cells.sum(),
                                                                                            (flagged & ok).sum(), float(excess.max())))
        assert (excess <= 1).all(), int((excess > 1).sum())
        assert (np.abs(rep[0] - g["q"])[ok] > tol(A[0][ok])).mean() > 0.9
        # the statistics are the matrix's
        assert np.array_equal(g["support"], np.where(ok, (rep > 0).sum(axis=0), 0))
        assert np.array_equal(g["q_sum"], np.where(ok, rep.sum(axis=0), 0))
        assert np.array_equal(g["q_min"], np.where(ok, rep.min(axis=0), 0))
        assert np.array_equal(g["q_max"], np.where(ok, rep.max(axis=0), 0))
    for k in got["fresh"]:
        assert np.array_equal(got["fresh"][k], got["stepped"][k]), k
