"""GPU: the engine, through the C ABI, against outputs RECORDED from the reference's own kernels (tests/golden/ref_mutations.npz,
ref_likelihood.npz; written by tests/golden/make_ref_fixtures.py from oracle/ref_kernels.py, cases of tests/ref_cases.py) -- no
restatement of the reference between the engine and the reference's program text.  Inputs are regenerated from their seeds and held
to the digests the fixtures carry.

Tolerances are the ones the suite already uses for the same quantities against the oracle: fragment layouts equal as integers;
full logL rel 1e-8 (test_repeats_gpu.py, smoke()); candidate deltas 2e-9 |logL| (smoke()) and 1e-7 |logL| with repeated bins
(test_candidate_deltas_with_repeats).

fA == fB is the one place where the engine deliberately does not follow the reference, and
both halves of that deviation are asserted here against the recorded reference, not skipped:
* graal_apply_move: the ten candidates that involve fB leave the layout alone (the reference pastes / inserts the fragment
  next to itself); ops 0, 1 and 8 act on fA and equal the reference;
* graal_eval_candidates: a neighbour equal to fA scores 0 for ALL 13 candidates, ops 0, 1 and 8 included, although the
  reference's sub_compute_likelihood gives them finite, mostly nonzero values (the fixture holds them; e.g. lin_1sub_grid
  fA = 9: op 0 = op 8 = -2.2808; circ_1sub_generic fA = 19: op 0 = -29.59).  The test asserts the zeros AND that the
  reference's values exist, so the deviation cannot grow or vanish unnoticed.
Each test prints its worst |engine - reference| / tolerance.
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import ref_cases as C
from tests.test_engine_gpu import engine_for
from tests.test_repeats_gpu import engine_with_repeats

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MUT = np.load(os.path.join(HERE, "golden", "ref_mutations.npz"))
LIK = np.load(os.path.join(HERE, "golden", "ref_likelihood.npz"))
LAYOUT_IDS = [lay["name"] for lay in C.LAYOUTS]


def engine_of(lay):
    """The layout on the device, in reference arithmetic, relabelled (labels are ranks already: nothing moves)."""
    e = (engine_with_repeats if lay["repeats"] else engine_for)(lay["P"], lay["state"])
    e.set_mode(ref_trans_accu=True, strict=True)
    assert e.relabel_contigs() == lay["max_id"]
    got = e.download_frags()
    for k in O.FIELDS:
        assert np.array_equal(got[k], lay["state"][k]), k
    return e


def test_case_list_is_the_recorded_one():
    assert all(C.CLASS_COUNTS[c] >= 8 for c in C.CLASSES), C.CLASS_COUNTS
    assert [int(d) for d in MUT["digest"]] == [lay["digest"] for lay in C.LAYOUTS]
    assert [int(d) for d in LIK["digest"]] == [lay["digest"] for lay in C.LAYOUTS]


@pytest.mark.parametrize("li", range(len(C.LAYOUTS)), ids=LAYOUT_IDS)
def test_apply_move_equals_the_reference_kernels(li):
    lay = C.LAYOUTS[li]
    s = lay["state"]
    out_f, wr_f, st_f = C.recorded_candidates(MUT, li)
    pairs = [(fA, fB) for fA, fBs in lay["proposals"] for fB in fBs]
    assert len(pairs) == len(out_f)
    e = engine_of(lay)
    refused = mismatches = 0
    for i, (fA, fB) in enumerate(pairs):
        for op in range(C.N_OPS):
            e.upload_frags(s)
            assert e.relabel_contigs() == lay["max_id"]
            n_stale = e.apply_move(fA, fB, op, lay["max_id"])
            got = e.download_frags()
            if fA == fB and op in C.OPS_NEEDING_FB:      # the documented deviation: a no-op (ops 0, 1, 8 are compared below)
                assert n_stale == 0 and all(np.array_equal(got[k], s[k]) for k in O.FIELDS), (fA, op)
                refused += 1
                continue
            assert n_stale == st_f[i, op], (fA, fB, op, n_stale, st_f[i, op])
            w = wr_f[i, op]
            for j, k in enumerate(O.FIELDS):
                bad = int((got[k][w] != out_f[i, op, j][w]).sum())
                mismatches += bad
                assert bad == 0, (lay["name"], fA, fB, op, k)
    e.close()
    assert refused == len(C.OPS_NEEDING_FB) * sum(1 for fA, fB in pairs if fA == fB)
    print("\n[ref] %s: %d candidates, %d refused (fA == fB), mismatching entries %d" %
          (lay["name"], len(pairs) * C.N_OPS, refused, mismatches))


@pytest.mark.parametrize("li", range(len(C.LAYOUTS)), ids=LAYOUT_IDS)
def test_full_evaluation_equals_the_reference_kernels(li):
    lay = C.LAYOUTS[li]
    want = float(LIK["l%d_total" % li])
    assert want == pytest.approx(float(np.sum(LIK["l%d_pixels" % li])), rel=1e-12)
    e = engine_of(lay)
    got = e.eval_full()
    e.close()
    print("\n[ref] %s: full logL %.9f, |engine - reference| / (1e-8 |logL|) = %.3g" %
          (lay["name"], want, abs(got - want) / (1e-8 * abs(want))))
    assert got == pytest.approx(want, rel=1e-8)


@pytest.mark.parametrize("li", range(len(C.LAYOUTS)), ids=LAYOUT_IDS)
def test_candidate_deltas_equal_the_reference_kernels(li):
    lay = C.LAYOUTS[li]
    base = float(LIK["l%d_total" % li])
    deltas_f = LIK["l%d_deltas" % li]
    assert deltas_f.shape == (len(lay["proposals"]), C.K, C.N_OPS)
    tol = (1e-7 if lay["repeats"] else 2e-9) * abs(base)
    _, _, st_f = C.recorded_candidates(MUT, li)
    e = engine_of(lay)
    worst = self_worst = 0.0
    n_self = 0
    for i, (fA, fBs) in enumerate(lay["proposals"]):
        pair0 = i * C.K
        got = e.eval_candidates(fA, fBs, lay["max_id"])
        for k, fB in enumerate(fBs):
            if fB == fA:
                # the documented deviation: the engine scores a neighbour equal to fA as 0 for all
                # 13 candidates; the reference prices every one it can write (stale pastes are the NaNs), ops 0 / 1 / 8 always
                assert np.all(got[k] == 0), (fA, got[k])
                assert np.all(np.isfinite(deltas_f[i, k][[0, 1, 8]])), (fA, deltas_f[i, k])
                assert np.array_equal(np.isnan(deltas_f[i, k]), st_f[pair0 + k] > 0)
                n_self += 1
                self_worst = max(self_worst, float(np.nanmax(np.abs(deltas_f[i, k]))))
                continue
            assert not np.any(np.isnan(deltas_f[i, k])), "only a candidate of fA with itself is stale in the reference"
            err = np.abs(got[k] - deltas_f[i, k])
            worst = max(worst, float(err.max()) / tol)
            assert np.all(err <= tol), (lay["name"], fA, fB, err.max(), tol, got[k] - deltas_f[i, k])
    e.close()
    print("\n[ref] %s: %d proposals x %d candidates, worst |engine - reference| / tolerance = %.3g (tolerance %.3g); "
          "%d neighbours equal to fA scored 0 by the engine, largest reference |delta| among them %.4f" %
          (lay["name"], len(lay["proposals"]), C.K * C.N_OPS, worst, tol, n_self, self_worst))
