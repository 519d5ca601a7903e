"""The numpy restatement of graal_junction_bootstrap (tests/junction_boot_reference.py) checked on its own, without a GPU: its split into
mass and contacts against tests/junction_reference.py, its draws against tests/sim_reference.py's scalar sampler, what a replicate may
and may not depend on, the Poisson mean of the contact part, and the condition the GPU tests lean on -- few flagged cells in every case
and seed they use."""
import numpy as np
import pytest

from tests import junction_boot_reference as BR
from tests import junction_reference as JR
from tests import sim_reference as SR


@pytest.mark.parametrize("name,quirk", [(n, q) for n, q, _ in BR.SMALL_CASES])
def test_counts_for_draws_give_the_junction_scores(name, quirk):
    """With the draw replaced by the count itself: junction_reference.junction_scores exactly -- J, the statuses and the sums of |terms|."""
    P = BR.small_case(name)
    B = BR.small_boot(name, quirk)
    J, A, nf = B.score(B.ob)
    Jr, st, Ar = JR.reference(P, quirk=quirk)
    assert np.array_equal(B.status, st) and not nf.any()
    assert (st == JR.VALID).sum() >= 10
    assert np.array_equal(J, Jr) and np.array_equal(A, Ar)
    mass_only = np.where(st == JR.VALID, B.M, 0)
    assert (mass_only != Jr).sum() >= 10                  # (the contacts carry a part of every score: the split is not vacuous)


def test_vectorised_draws_are_the_scalar_sampler():
    B = BR.small_boot("sub1", False)
    assert (B.ob < 10).sum() >= 100 and (B.ob >= 10).sum() >= 20 and (B.ob != np.rint(B.ob)).sum() == 1
    for r in (0, 3, 149):
        c, fl = BR.draw_counts(B.row, B.col, B.ob, 8, r)
        for i in range(len(c)):
            st = SR.Stream(B.row[i], B.col[i], 2 | (r << 8), 8)
            assert SR.poisson(float(B.ob[i]), st) == c[i] and st.flag == fl[i], (r, i)
    assert (c != np.rint(B.ob)).sum() > len(c) // 2
    # a count of 0 or below draws 0 and flags nothing
    c, fl = BR.draw_counts([1, 2], [3, 4], [0.0, -2.0], 8, 0)
    assert not c.any() and not fl.any()


def test_what_a_replicate_depends_on():
    name, quirk, seed = BR.SMALL_CASES[0]
    B = BR.small_boot(name, quirk)
    few, many = B.replicates(seed, range(3)), B.replicates(seed, range(11))
    for x, y in zip(few, many):
        assert np.array_equal(x, y[:3])                   # replicate r is the same whatever n_rep
    other = B.replicates(seed + 1, range(3))
    ok = B.status == BR.VALID
    assert (other[0][:, ok] != few[0][:, ok]).mean() > 0.9
    assert (few[0][0, ok] != few[0][1, ok]).mean() > 0.9  # ... and differs from the next one
    P = dict(BR.small_case(name))
    perm = np.random.RandomState(4).permutation(len(P["coo_row"]))
    for k in ("coo_row", "coo_col", "coo_val"):
        P[k] = np.asarray(P[k])[perm]
    shuffled = BR.boot(P, quirk=quirk).replicates(seed, range(3))
    for x, y in zip(few, shuffled):
        assert np.array_equal(x, y)                       # the draw belongs to (row, col), not to the place in the list


def test_mean_contact_part_is_the_data_s():
    """400 replicates: the mean contact part lies within 5 sigma / sqrt(400) of the data's own at every valid junction, sigma^2 = the sum
    of ob * t^2 over the straddling contacts (a Poisson count's variance is its mean)."""
    R = 400
    B = BR.boot(JR.case("sub3"))
    ok = B.status == BR.VALID
    data = B.straddle(B.terms(B.ob)[0]).astype(np.float64)
    var = np.zeros(B.n + 1)
    w = B.ob * (B.t * BR.Q) ** 2
    np.add.at(var, B.lo, w); np.add.at(var, B.hi, -w)
    sigma = np.sqrt(np.maximum(np.cumsum(var)[B.slot], 0.0))
    mean = np.zeros(B.n)
    for r in range(R):
        c, _ = BR.draw_counts(B.row, B.col, B.ob, 21, r)
        mean += B.straddle(B.terms(c)[0])
    mean /= R
    assert ok.sum() >= 40 and (sigma[ok] > 0).sum() >= 40
    z = np.abs(mean[ok] - data[ok]) / (sigma[ok] / np.sqrt(R) + 1.0)          # (+ 1 Q: the terms' own rounding)
    print("largest |mean - data| in sigma / sqrt(R): %.2f" % z.max())
    assert (z <= 5.0).all(), z.max()
    assert (np.abs(mean[ok] - data[ok]) > 0).all()


def test_few_cells_are_flagged_in_the_cases_the_gpu_tests_use():
    for name, quirk, seed in BR.SMALL_CASES:
        B = BR.small_boot(name, quirk)
        _, _, fl, nf = BR.small_replicates(name, quirk, seed)
        ok = B.status == BR.VALID
        assert not nf.any()
        assert fl[:, ok].sum() <= 0.02 * ok.sum() * len(BR.REF_REPS), (name, quirk, seed, int(fl.sum()))


@pytest.mark.parametrize("quirk", [False, True])
def test_few_cells_are_flagged_at_mid_size(quirk):
    B, (_, _, fl, nf) = BR.mid_replicates(quirk)
    ok = B.status == BR.VALID
    assert ok.sum() >= 2990 and not nf.any()
    assert fl[:, ok].sum() <= 0.02 * ok.sum() * BR.MID_REPS, int(fl.sum())
