"""The numpy restatement of graal_end_links_bootstrap (tests/link_boot_reference.py) checked on its own, without a GPU: its split into
mass and contacts against tests/link_reference.py, its draws against tests/sim_reference.py's scalar sampler under the junction
bootstrap's tag, what a replicate may and may not depend on, the mutual rule on a hand-built table, the Poisson mean of the contact part,
the table helpers, the entry points' refusal on a handle without a device, and the condition the GPU tests lean on -- few flagged cells
in every case and seed they use."""
import ctypes

import numpy as np
import pytest

from graal_amd import links
from graal_amd.lib import Engine, GraalError
from tests import junction_boot_reference as BR
from tests import link_boot_reference as KR
from tests import link_reference as LR
from tests import sim_reference as SR


@pytest.mark.parametrize("name,quirk,min_frags", [c[:3] for c in KR.SMALL_CASES])
def test_counts_for_draws_give_the_links(name, quirk, min_frags):
    """With the draw replaced by the count itself: link_reference's links() exactly -- the listed set, L, the statuses, the sums of |terms|."""
    P = KR.small_case(name)
    B = KR.small_boot(name, quirk, min_frags)
    L, A, st = B.score(B.R.count)
    ra, rb, rq, _, rst, rA = LR.restatement(P, quirk=quirk).links(P["S_o_A_frags"], min_frags)
    assert len(ra) >= 10 and np.array_equal(B.end_a, ra) and np.array_equal(B.end_b, rb)
    assert np.array_equal(st, rst) and (st == KR.VALID).all()
    assert np.array_equal(L, rq) and np.array_equal(A, rA)
    assert (B.mass != rq).sum() >= 10                     # (the contacts carry a part of every score: the split is not vacuous)


def test_cases_hold_both_sampler_branches_the_fill_and_the_mirror():
    for name, quirk, min_frags, _ in KR.SMALL_CASES:
        B = KR.small_boot(name, quirk, min_frags)
        ob = B.R.count[B.used]
        assert (ob < 10).sum() >= 10 and len(ob) >= 15, name  # (the ring case at min_frags 2 is the smallest: 17 contacts)
        if min_frags == 1:
            assert np.isin(ob, KR.PLANTED).sum() >= len(KR.PLANTED) and (ob != np.rint(ob)).sum() == 1, name
    # with the indexing mode on, links re-price contacts against third contigs: the mirror's contact part is in the cases
    P = KR.small_case("sub3")
    B = KR.small_boot("sub3", True, 1)
    lab = np.asarray(P["S_o_A_frags"]["id_c"])
    idc = lab[B.R.bin_of]
    third = 0
    for i in range(B.m):
        ca, cb = lab[B.end_a[i] >> 1], lab[B.end_b[i] >> 1]
        s, t = B.sel[i], B.t[i]
        r, c = B.R.row[s], B.R.col[s]
        outside = ~(np.isin(idc[r], (ca, cb)) & np.isin(idc[c], (ca, cb)))
        third += int((outside & (t != 0.0)).sum())
    assert B.R.mixed.sum() >= 5 and third >= 20, third


def test_draws_are_the_junction_bootstrap_s():
    """The same (row, col, r, seed) draws the same count as the junction restatement's stream: tag 2 | r << 8, the scalar sampler."""
    B = KR.small_boot("sub1", False, 1)
    k = np.nonzero(B.used)[0]
    for r in (0, 3, 149):
        c, fl = B.draws(8, r)
        jc, jf = BR.draw_counts(B.R.row[k], B.R.col[k], B.R.count[k], 8, r)
        assert np.array_equal(c[k], jc) and np.array_equal(fl[k], jf)
        for i in k[:200]:
            st = SR.Stream(B.R.row[i], B.R.col[i], 2 | (r << 8), 8)
            assert SR.poisson(float(B.R.count[i]), st) == c[i] and st.flag == fl[i], (r, i)
        assert not c[~B.used].any() and not fl[~B.used].any()
    assert (c[k] != np.rint(B.R.count[k])).sum() > len(k) // 3


def test_what_a_replicate_depends_on():
    name, quirk, min_frags, seed = KR.SMALL_CASES[0]
    B = KR.small_boot(name, quirk, min_frags)
    few, many = B.replicates(seed, range(3)), B.replicates(seed, range(11))
    for x, y in zip(few, many):
        assert np.array_equal(x, y[:3])                   # replicate r is the same whatever n_rep
    other = B.replicates(seed + 1, range(3))
    # (a link that rests on a single contact of count 1 redraws the same count about one time in three: not every cell differs)
    assert (other[0] != few[0]).mean() > 0.6
    assert (few[0][0] != few[0][1]).mean() > 0.6          # ... and differs from the next one
    P = dict(KR.small_case(name))
    perm = np.random.RandomState(4).permutation(len(P["coo_row"]))
    for k in ("coo_row", "coo_col", "coo_val"):
        P[k] = np.asarray(P[k])[perm]
    shuffled = KR.LinkBoot(LR.restatement(P, quirk=quirk), P["S_o_A_frags"], min_frags).replicates(seed, range(3))
    for x, y in zip(few, shuffled):
        assert np.array_equal(x, y)                       # the draw belongs to (row, col), not to the place in the list


def test_mutual_on_a_hand_built_table_with_a_tie():
    """Three ends 2, 5, 9 and all three links.  Row 0: end 2 scores 7 with both 5 and 9 -- the tie goes to the lower partner, 5; 5's best
    is 2: (2, 5) is mutual, (2, 9) is not, and 9's best is 2 (7 > 3), so (5, 9) is not.  Row 1: (5, 9) is the best of both its ends.  Row
    2: the mutual link (2, 9) scores 4, not above a threshold of 4.  Row 3 without its middle link (not valid): end 5 scores 5 with both 2
    and 9, the tie goes to 2, whose only link that is: (2, 5) is mutual."""
    a, b = np.array([2, 2, 5]), np.array([5, 9, 9])
    rep = np.array([[7, 7, 3], [1, 2, 8], [1, 4, 2], [5, 9, 5]])
    ok = np.array([True, True, True])
    assert KR.mutual_counts(a, b, rep[:1], ok).tolist() == [1, 0, 0]
    assert KR.mutual_counts(a, b, rep[1:2], ok).tolist() == [0, 0, 1]
    assert KR.mutual_counts(a, b, rep[2:3], ok, threshold=4).tolist() == [0, 0, 0]
    assert KR.mutual_counts(a, b, rep[2:3], ok, threshold=3).tolist() == [0, 1, 0]
    assert KR.mutual_counts(a, b, rep, ok).tolist() == [1, 2, 1]
    assert KR.mutual_counts(a, b, rep[3:], np.array([True, False, True])).tolist() == [1, 0, 0]
    # the table helpers' rule is the same one
    soa = {"id_c": np.arange(6)}
    t = links.table_from(soa, a, b, [1, 1, 1], rep[0].astype(float))
    m = links.mutual_best(t)
    assert list(2 * m["frag_a"] + m["side_a"]) == [2] and list(2 * m["frag_b"] + m["side_b"]) == [5]


def test_mean_contact_part_is_the_data_s():
    """400 replicates: the mean contact part lies within 5 sigma / sqrt(400) of the data's own at every valid link, sigma^2 = the sum of
    ob * t^2 over the link's contacts (a Poisson count's variance is its mean)."""
    R = 400
    P = LR.case("sub3")
    B = KR.LinkBoot(LR.restatement(P, quirk=True), P["S_o_A_frags"], 1)
    data = B.contact_part(B.R.count)
    sigma = np.sqrt(B.contact_var())
    mean = np.zeros(B.m)
    for r in range(R):
        mean += B.contact_part(B.draws(21, r)[0])
    mean /= R
    assert B.m >= 40 and (sigma > 0).all()
    z = np.abs(mean - data) / (sigma / np.sqrt(R))
    print("largest |mean - data| in sigma / sqrt(R): %.2f" % z.max())
    assert (z <= 5.0).all(), z.max()
    assert (np.abs(mean - data) > 0).all()


def test_few_cells_are_flagged_in_the_cases_the_gpu_tests_use():
    for name, quirk, min_frags, seed in KR.SMALL_CASES:
        B = KR.small_boot(name, quirk, min_frags)
        _, _, fl, st = KR.small_replicates(name, quirk, min_frags, seed)
        assert (st == KR.VALID).all()
        assert set(KR.DEFINING_REPS) <= set(KR.REF_REPS) and KR.REF_REPS[-1] == KR.N_REP - 1
        assert fl.sum() <= 0.02 * B.m * len(KR.REF_REPS), (name, quirk, min_frags, seed, int(fl.sum()))


def _support_table():
    soa = {"id_c": np.array([3, 3, 5, 5, 5, 8])}
    t = links.table_from(soa, [1, 1], [4, 6], [10, 4], [5.0, np.nan])
    t.update({"support": np.array([0.75, np.nan]), "mutual": np.array([0.5, np.nan]), "boot_mean": np.array([4.5, np.nan]),
              "boot_min": np.array([-1.0, np.nan]), "boot_max": np.array([9.25, np.nan])})
    return t


def test_support_tsv(tmp_path):
    assert links.SUPPORT_COLUMNS[:len(links.COLUMNS)] == links.COLUMNS
    assert links.SUPPORT_COLUMNS[len(links.COLUMNS):] == ("support", "mutual", "boot_mean", "boot_min", "boot_max")
    p = tmp_path / "link_support.tsv"
    assert links.write_support_tsv(str(p), _support_table()) == 2
    lines = p.read_text().splitlines()
    assert lines[0].split("\t") == list(links.SUPPORT_COLUMNS)
    assert lines[1].split("\t") == ["3", "0", "1", "5", "2", "0", "10", "5.0", "0.75", "0.5", "4.5", "-1.0", "9.25"]
    assert lines[2].split("\t")[7:] == ["nan"] * 6


def test_bootstrap_refuses_without_gpu():
    """graal_end_links_bootstrap, its fetch and Engine.end_links_bootstrap on a handle without a device: an error, nothing computed on
    the host, outputs untouched."""
    from graal_amd import build as gbuild
    from graal_amd import lib
    gbuild.build_hip()
    L = lib.load()
    h = ctypes.c_void_p()
    if L.graal_create(0, ctypes.byref(h)) == 0:
        L.graal_destroy(h)
        pytest.skip("a GPU is present: tests/test_links_bootstrap_gpu.py covers the engine")
    try:
        m = ctypes.c_int64(7)
        rc = L.graal_end_links_bootstrap(h, 1, ctypes.c_uint64(3), 5, 0, 1, ctypes.byref(m))
        assert rc != 0 and L.graal_last_error(h).decode() and m.value == 7
        a, s = np.full(4, 7, np.int32), np.full(4, 7, np.int32)
        q = np.full(4, 7, np.int64)
        st = np.full(4, 9, np.uint8)
        i32, i64 = lambda x: x.ctypes.data_as(lib._i32p), lambda x: x.ctypes.data_as(lib._i64p)
        rc = L.graal_end_links_bootstrap_fetch(h, i32(a), i32(a), i64(q), i64(q), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), i32(s),
                                               i32(s), i64(q), i64(q), i64(q), None, 4)
        assert rc != 0 and (a == 7).all() and (s == 7).all() and (q == 7).all() and (st == 9).all()
        e = Engine.__new__(Engine)
        e._L, e._h, e.n = L, h, 4
        with pytest.raises(GraalError, match="graal_end_links_bootstrap"):
            e.end_links_bootstrap(3, 5)
        with pytest.raises(GraalError, match="graal_end_links_bootstrap"):
            links.support_table(e, 3, 5)
        e._h = None
    finally:
        L.graal_destroy(h)


@pytest.mark.parametrize("quirk", [False, True])
def test_mid_size_restatement_and_its_flags(quirk):
    """tests/window_cases.m2 as the mid-size GPU test uses it: with the count itself for the draw the windowed restatement's own links
    exactly, every link valid, and few flagged cells under the seed that test uses."""
    from tests import window_reference as WR
    P = BR.mid_case()
    B, (_, _, fl, st) = KR.mid_replicates(quirk)
    W = WR.window(P, quirk)
    a, b, q, _, rst, A = W.links(P["S_o_A_frags"], KR.MID_MIN_FRAGS)
    L0, A0, st0 = B.score(W.count)
    assert B.m >= 20 and np.array_equal(a, B.end_a) and np.array_equal(b, B.end_b)
    assert np.array_equal(L0, q) and np.array_equal(A0, A) and np.array_equal(st0, rst) and (st == KR.VALID).all()
    assert fl.sum() <= 0.02 * B.m * KR.MID_REPS, int(fl.sum())
    if quirk:
        assert max(len(s) for s in B.sel) > 2000          # (the contacts against third contigs: the mirror's contact part)
