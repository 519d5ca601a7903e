"""graal_end_links_bootstrap at a mid-size shape: tests/window_cases.m2 as the junction bootstrap uses it (contigs of 500 .. 1,100 bins,
each above 1,024 bins or longer than the contact window; n_sub 3, mixed RF counts, reversed bins; 119,999 row-sorted contacts, so the
last wave is short and rows' contacts span two waves: runs of equal links cross lane 63), on a fresh engine and on a stepped one, eight
replicates, against the windowed restatement (tests/link_boot_reference.WindowLinkBoot on tests/window_reference.py)."""
import numpy as np
import pytest

from graal_amd.lib import LINK_VALID
from tests import junction_boot_reference as BR
from tests import link_boot_reference as KR
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
    B, (L, A, flagged, rst) = KR.mid_replicates(quirk)
    got = {}
    for engine_state in ("fresh", "stepped"):
        e, s, Sw = engine_in(engine_state, P, quirk=quirk)
        try:
            table = e.end_links_q(KR.MID_MIN_FRAGS)
            g = e.end_links_bootstrap_q(KR.MID_SEED, KR.MID_REPS, KR.MID_MIN_FRAGS, 0, replicates=True)
        finally:
            e.close()
        got[engine_state] = g
        assert (s["l_cont"] > 1024).any()
        # the data's own columns, word for word; the listed set is the restatement's
        for col, want in zip(("end_a", "end_b", "q", "contacts", "status"), table):
            assert np.array_equal(g[col], want), col
        assert np.array_equal(g["end_a"], B.end_a) and np.array_equal(g["end_b"], B.end_b) and B.m >= 20
        assert (g["status"] == LINK_VALID).all() and (rst == KR.VALID).all()
        # the replicates
        rep = g["q_rep"]
        assert rep.shape == L.shape
        cells = ~flagged
        assert cells.sum() >= 0.98 * B.m * KR.MID_REPS
        excess = np.abs(rep - L)[cells] / tol(A[cells])
        print("m2 quirk %d %s: %d cells, %d flagged, largest |q_rep - L*| / tolerance %.3e" % (quirk, engine_state, cells.sum(),
                                                                                            flagged.sum(), float(excess.max())))
        assert (excess <= 1).all(), int((excess > 1).sum())
        assert (np.abs(rep[0] - g["q"]) > tol(A[0])).mean() > 0.9
        # the statistics are the matrix's
        assert np.array_equal(g["support"], (rep > 0).sum(axis=0))
        assert np.array_equal(g["q_sum"], rep.sum(axis=0))
        assert np.array_equal(g["q_min"], rep.min(axis=0)) and np.array_equal(g["q_max"], rep.max(axis=0))
        assert np.array_equal(g["mutual"], KR.mutual_counts(g["end_a"], g["end_b"], rep, g["status"] == LINK_VALID))
    for k in got["fresh"]:
        assert np.array_equal(got["fresh"][k], got["stepped"][k]), k
