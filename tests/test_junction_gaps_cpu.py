"""Junction gaps without a GPU: the numpy restatement (tests/junction_gap_reference.py) against its own consequences (zeros at gap 0,
minus the junction score at gaps >= d_max, no part for the trans-branch indexing), against the sparse scorer's full likelihood of the
layout with the right part moved, on simulated data with planted gaps, and the table, its TSV file and the default grid."""
import numpy as np
import pytest

from graal_amd import junctions
from oracle.sparse_numpy import SparseScorer
from tests import junction_gap_reference as GR
from tests import junction_reference as JR
from tests import window_reference as WR

CASES = ["sub3", "sub1", "circ"]


@pytest.mark.parametrize("name", CASES)
def test_zero_gap_is_zero_and_a_window_wide_gap_is_a_cut(name):
    P, grid, G, st, A = GR.small(name)
    J, st_j, _ = JR.reference(P, quirk=False)
    d_max = np.float32(P["param_simu"][5])
    assert grid[0] == 0 and not G[0].any() and not A[0].any()
    wide = np.nonzero(grid >= d_max)[0]
    assert len(wide) == 2 and grid[wide[0]] == d_max
    for g in wide:
        assert np.array_equal(G[g], -J)
    assert np.array_equal(st, st_j) and (st == GR.VALID).sum() >= 10
    s = P["S_o_A_frags"]
    assert (st[np.asarray(s["circ"]) == 1] == GR.CIRCULAR).all() and ((st == GR.CIRCULAR).any() == (name == "circ"))
    ok = st == GR.VALID
    assert not G[:, ~ok].any()
    for g in range(len(grid) - 2):
        assert (G[g][ok] != G[g + 1][ok]).all(), g                  # every grid value is a different question


@pytest.mark.parametrize("name", CASES)
def test_two_restatements_agree_and_the_mode_flag_plays_no_part(name):
    """Brute force over the pairs of every junction equals the vectorised, windowed restatement word for word; the latter under the
    trans-branch indexing is the same (the pairs stay cis)."""
    P, grid, G, st, A = GR.small(name)
    for quirk in (False, True):
        G2, st2, A2 = GR.Gaps(WR.window(P, quirk)).profiles(P["S_o_A_frags"], grid)
        assert np.array_equal(G, G2) and np.array_equal(st, st2) and np.array_equal(A, A2), quirk
    if name == "sub3":                                               # (where the indexing does move the junction scores)
        assert not np.array_equal(JR.reference(P, quirk=True)[0], JR.reference(P, quirk=False)[0])


@pytest.mark.parametrize("name", CASES)
def test_reference_equals_full_likelihood_of_the_moved_layout(name):
    """G = full(layout with the right part's start_bp moved g bp) - full(layout) by the sparse scorer, the layout un-recentred as
    junction_reference.cut_layout(recentre=False) leaves it, for gaps of 137, 2,500 and 40,000 bp.  Two kinds of rounding noise, both
    measured here (printed).
    Inside the right part: its centres are recomputed as f32((start + g) / 1000) + ..., so the distances between its OWN sub-fragments
    move by float32 last places of a coordinate -- pairs the gap does not touch by definition.  The same scorer prices that alone: the
    right part cut off (un-recentred) and moved, minus cut off and not moved; up to 2.9 log units here (3e-2 of the terms).  It is
    taken out of the difference.
    Across the junction: the distance is |f32 centre_b' - centre_a|, not f32(sd + g).  For 2.5 and 40 kb (float32 values, and sums that
    stay on the coordinates' float32 grid) what is left meets the junction scores' 1e-7 of the terms (measured: 5.6e-8; the scorer's
    own float32 np.power is not correctly rounded).  0.137 kb is no float32 value and falls between the last places (7.6e-6 kb at
    100 kb) of the coordinates it is added to; neighbours across the junction are ~0.1 kb apart and the price goes as sd^slope, so a
    term moves by up to slope * 7.6e-6 / 0.1 ~ 1e-4 of itself; measured 7.5e-6 of the sum of |terms|, bound 1e-5."""
    P, _, _, st, _ = GR.small(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    gaps_bp = ((137, 1e-5), (2500, 1e-7), (40000, 1e-7))
    G, st2, A = GR.reference(P, [g / 1000.0 for g, _ in gaps_bp])
    assert np.array_equal(st, st2)
    valid = np.nonzero(st == GR.VALID)[0]
    base = sp.full(s)
    worst, worst_inside = [0.0] * len(gaps_bp), 0.0
    for f in valid[:: max(1, len(valid) // 5)]:
        right = (s["id_c"] == s["id_c"][f]) & (s["pos"] > s["pos"][f])
        cut = JR.cut_layout(s, int(f), recentre=False)
        for k, (g, bound) in enumerate(gaps_bp):
            moved = {key: v.copy() for key, v in s.items()}
            moved["start_bp"][right] += g
            cut_moved = {key: v.copy() for key, v in cut.items()}
            cut_moved["start_bp"][right] += g
            inside = sp.full(cut_moved) - sp.full(cut)
            want = sp.full(moved) - base - inside
            got = G[k, f] / GR.Q
            a = A[k, f] / GR.Q
            worst[k] = max(worst[k], abs(got - want) / a)
            worst_inside = max(worst_inside, abs(inside))
            assert abs(got - want) <= bound * a + 1e-6, (f, g, got, want, inside, a)
    print("%s: largest |G - (full(moved) - full - inside)| / sum of |terms| per gap %s; largest inside noise %.3g log units"
          % (name, ["%.2e" % w for w in worst], worst_inside))
    assert (G[:, valid] != 0).any()


def test_simulated_gaps_lie_inside_their_intervals():
    """The 1,000-bin genome with contacts drawn (numpy Poisson) from its true layout; runs of 3, 10 and 30 bins taken out of contig 0
    and the hole closed.  Each true gap lies inside [lo, hi] at drop 1.92, and at least 95 % of the untouched junctions (true gap 0)
    keep grid index 0 inside theirs."""
    P, true, test, planted = GR.simulated()
    W0 = WR.window(dict(P, coo_row=np.zeros(0, np.int64), coo_col=np.zeros(0, np.int64), coo_val=np.zeros(0)))
    n = W0.n
    idc, pos = np.asarray(true["id_c"], np.int64), np.asarray(true["pos"], np.int64)
    start, length = np.asarray(true["start_bp"], np.int64), np.asarray(true["len_bp"], np.int64)
    C = W0.centres(np.arange(n), start, np.asarray(true["ori"]) == 1)
    sid = np.asarray(P["np_sub_frags_id"], np.int64).reshape(-1, 4)[:, 0]
    rng = np.random.RandomState(2024)
    rows, cols, vals = [], [], []
    for _, m in WR._runs(idc, pos):
        for ii, jj, _ in W0._window_pairs(start[m], start[m] + length[m]):
            X, Y = m[ii], m[jj]
            lam = W0.cis(W0.acc_s[X, 0], W0.acc_s[Y, 0], np.abs(C[Y, 0] - C[X, 0]).astype(np.float32)).astype(np.float64)
            v = rng.poisson(lam)
            keep = v > 0
            rows.append(sid[X][keep]); cols.append(sid[Y][keep]); vals.append(v[keep])
    Pc = dict(P, coo_row=np.concatenate(rows), coo_col=np.concatenate(cols), coo_val=np.concatenate(vals).astype(np.float64))
    G, st, _ = GR.vectorised(Pc, GR.STAT_GRID, test)
    inside, share, rows = GR.check_simulated(G, st, test, planted)
    print("planted (gap, best, lo, hi kb):", [tuple(round(x, 2) for x in r) for r in rows], "share of true junctions holding 0: %.4f" % share)
    assert (st == GR.VALID).sum() == 1000 - 6 and len(GR.STAT_GRID) == 41
    assert all(inside), rows
    assert share >= 0.95, share


def test_fold_is_argmax_and_the_interval_within_the_drop():
    G = np.array([[0, 0, 0, 5], [3, -1, 0, 5], [3, -4, 0, 1], [1, -9, 0, 7]], np.int64)
    st = np.array([0, 0, 1, 0], np.uint8)
    best, qb, lo, hi = GR.fold(G, st, 0)
    assert list(best) == [1, 0, 0, 3] and list(qb) == [3, 0, 0, 7] and list(lo) == [1, 0, 0, 3] and list(hi) == [2, 0, 0, 3]
    best, qb, lo, hi = GR.fold(G, st, 2)
    assert list(lo) == [1, 0, 0, 0] and list(hi) == [3, 1, 0, 3]
    assert best.dtype == np.int32 and qb.dtype == np.int64


def test_default_grid():
    g = junctions.default_gap_grid(41.5, median_bin_kb=0.68)
    assert g.dtype == np.float32 and len(g) == 32 and g[0] == 0 and g[1] == np.float32(0.17) and g[-1] == np.float32(41.5)
    assert (np.diff(g) > 0).all() and np.allclose(g[2:] / g[1:-1], g[2] / g[1], rtol=1e-5)
    g = junctions.default_gap_grid(100.0, points=5, min_kb=1.0)
    assert np.allclose(g, [0, 1, 10 ** (2 / 3), 10 ** (4 / 3), 100], rtol=1e-6)
    assert list(junctions.default_gap_grid(8.0, points=2, min_kb=1.0)) == [0.0, 8.0]
    for bad in (dict(points=1, min_kb=1.0), dict(points=65, min_kb=1.0), dict(min_kb=0.0), dict(min_kb=50.0), dict()):
        with pytest.raises(ValueError):
            junctions.default_gap_grid(41.5, **bad)


def test_gap_table_and_tsv(tmp_path):
    soa = {"pos": np.array([1, 0, 0, 2, 1, 0]), "id_c": np.array([4, 4, 1, 4, 1, 7]), "next": np.array([3, 0, 4, -1, -1, -1]),
           "circ": np.zeros(6, int), "ori": np.array([1, -1, 1, 1, -1, 1]), "start_bp": np.array([100, 0, 0, 250, 40, 0]),
           "len_bp": np.array([150, 100, 40, 30, 60, 10])}
    grid = np.array([0.0, 0.5, 2.0, 8.0], np.float32)
    nan = np.nan
    gaps = {"J": np.array([1.5, -2.25, nan, nan, nan, nan]), "gap_kb": np.array([0.5, 8.0, nan, nan, nan, nan]),
            "gap_score": np.array([0.75, 2.25, nan, nan, nan, nan]), "gap_lo_kb": np.array([0.0, 2.0, nan, nan, nan, nan]),
            "gap_hi_kb": np.array([2.0, 8.0, nan, nan, nan, nan]), "best": np.array([1, 3, 0, 0, 0, 0], np.int32),
            "lo": np.array([0, 2, 0, 0, 0, 0], np.int32), "hi": np.array([2, 3, 0, 0, 0, 0], np.int32)}
    t = junctions.gap_table_from(soa, gaps, grid)
    assert tuple(t) == junctions.GAP_COLUMNS and junctions.GAP_COLUMNS[:len(junctions.COLUMNS)] == junctions.COLUMNS
    assert list(t["left_frag"]) == [2, 1, 0] and list(t["score"][1:]) == [-2.25, 1.5] and np.isnan(t["score"][0])
    assert list(t["gap_kb"][1:]) == [8.0, 0.5] and list(t["gap_lo_kb"][1:]) == [2.0, 0.0] and list(t["gap_hi_kb"][1:]) == [8.0, 2.0]
    assert list(t["gap_open"][1:]) == [1.0, 0.0] and np.isnan(t["gap_open"][0]) and list(t["gap_score"][1:]) == [2.25, 0.75]
    p = tmp_path / "junction_gaps.tsv"
    assert junctions.write_gaps_tsv(str(p), t) == 3
    lines = p.read_text().splitlines()
    assert lines[0].split("\t") == list(junctions.GAP_COLUMNS)
    assert lines[1].split("\t") == ["1", "0", "2", "4", "1", "-1", "40", "nan", "nan", "nan", "nan", "nan", "nan"]
    assert lines[2].split("\t") == ["4", "0", "1", "0", "-1", "1", "100", "-2.25", "8.0", "2.25", "2.0", "8.0", "1.0"]
    assert lines[3].split("\t") == ["4", "1", "0", "3", "1", "1", "250", "1.5", "0.5", "0.75", "0.0", "2.0", "0.0"]
