"""graal_block_swaps' numpy restatements against a dense likelihood and against each other, two flawed restatements that must miss, and
graal_amd.swaps' host logic (tilings, plan, edit, rounds) on hand-built cases.  No GPU."""
import numpy as np
import pytest

from graal_amd import swaps
from tests import edit_reference as ER
from tests import link_reference as LR
from tests import swap_reference as SR
from tests import window_cases
from tests.sim_reference import sub_records
from tests.test_flips_cpu import _RestatedEngine, _seventh_marks, _toy


def _whole(s):
    """One swap per linear contig of >= 2 fragments whose span is the whole contig, and in a ring one swap inside it."""
    circ = np.asarray(s["circ"])
    out = []
    for m in LR.contigs_of(s).values():
        if circ[m[0]] == 1 and len(m) > 3:
            out.append((m[1], m[1], m[3]))
        elif circ[m[0]] != 1 and len(m) >= 2:
            out.append((m[0], m[(len(m) - 1) // 2], m[-1]))
    return tuple(np.array(x, np.int32) for x in zip(*out))


def swap_sets(s, max_units=4):
    return list(swaps.tilings(s, None, max_units)) + [_whole(s)]


@pytest.mark.parametrize("name", ["sub3", "sub1", "circ"])
def test_brute_force_equals_dense_difference(name):
    """S = the difference of a dense sum over EVERY sub-fragment pair between the swapped layout, its pairs inside X, inside Y and
    inside the rest of the contig priced with their old centres, and the current layout (the flips' tolerance), for every swap of the
    tilings up to span 4 and the whole-contig spans; the same integers with the trans-branch indexing on and off.  The dense sum has
    no notion of which pairs a swap changes."""
    P = LR.case(name)
    s = P["S_o_A_frags"]
    R, Rq = SR.restatement(P, quirk=False), SR.restatement(P, quirk=True)
    centre = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], s)[0]
    base = {q: LR.dense_loglik(r, s, LR.pricer(r, s, centre)) for q, r in ((False, R), (True, Rq))}
    idc = np.asarray(s["id_c"])
    n_swaps, n_circ = 0, 0
    for i, (first, mid, last) in enumerate(swap_sets(s)):
        q, c, st, A = R.swaps(s, first, mid, last)
        for u, v in zip((q, c, st, A), Rq.swaps(s, first, mid, last)):
            assert np.array_equal(u, v)
        for k in range(len(first)):
            if st[k] == SR.CIRCULAR:
                assert q[k] == 0 and c[k] == 0 and np.asarray(s["circ"])[first[k]] == 1
                n_circ += 1
                continue
            assert st[k] == SR.VALID
            S = SR.swap_layout(s, first[k], mid[k], last[k])
            cS = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], S)[0]
            m, sx, sy = SR._members(s, int(first[k]), int(mid[k]), int(last[k]))
            fixed = []
            for g in (m[sx], m[sy], np.concatenate([m[:sx.start], m[sy.stop:]])):
                mask = np.zeros(R.n, bool); mask[g] = True
                fixed.append((mask[R.bin_of], centre))
            for quirk, r in ((False, R), (True, Rq)) if (k + i) % 7 == 0 else ((False, R),):
                d = LR.dense_loglik(r, S, LR.pricer(r, S, cS, fixed)) - base[quirk]
                assert abs(q[k] / LR.Q - d) <= 1e-7 * A[k] / LR.Q + 1e-6, (first[k], mid[k], last[k], q[k] / LR.Q, d)
            n_swaps += 1
    assert n_swaps >= (40 if name == "circ" else 100) and (n_circ > 0) == (name == "circ")   # (circ: a ring and few linear pieces)


@pytest.mark.parametrize("name,quirk", [("w1", False), ("w3", False), ("w3", True)])
def test_windowed_equals_brute_force(name, quirk):
    P = window_cases.small(name)
    s = P["S_o_A_frags"]
    B, W = SR.restatement(P, quirk=quirk), SR.window(P, quirk=quirk)
    sets = list(swaps.tilings(s, None, 3)) + list(swaps.tilings(s, _seventh_marks(s), 4))
    assert len(sets) == 8 + 20
    far = 0
    for first, mid, last in sets:
        got, want = W.swaps(s, first, mid, last), B.swaps(s, first, mid, last)
        for g, w, what in zip(got, want, ("q", "contacts", "status", "A")):
            assert np.array_equal(g, w), (what, np.nonzero(g != w)[0][:5])
        start, ln = np.asarray(s["start_bp"], np.int64), np.asarray(s["len_bp"], np.int64)
        sm = start[mid] + ln[mid]
        far += int((np.maximum(sm - start[first], start[last] + ln[last] - sm) > 2 * W.reach + 2000).sum())
    assert far > 0                                # (a run longer than two windows: its interior does not contribute)


def test_windowed_equals_brute_force_in_one_call_with_neighbouring_swaps():
    """Swaps of one call less than a window apart, with contacts between them: each carries its own term (only that swap applied)."""
    P = window_cases.small("w3")
    s = P["S_o_A_frags"]
    first, mid, last = next(iter(swaps.tilings(s, None, 3)))
    assert len(first) > 10
    got, want = SR.window(P).swaps(s, first, mid, last), SR.restatement(P).swaps(s, first, mid, last)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert (got[1] > 0).sum() > 10
    # contacts between two swaps of the call exist, and each of the two prices them
    bin_of = SR.restatement(P).bin_of
    sw = np.full(len(s["id_c"]), -1)
    pos, idc = np.asarray(s["pos"]), np.asarray(s["id_c"])
    for k, (f, l) in enumerate(zip(first, last)):
        sw[(idc == idc[f]) & (pos >= pos[f]) & (pos <= pos[l])] = k
    a, b = sw[bin_of[np.asarray(P["coo_row"])]], sw[bin_of[np.asarray(P["coo_col"])]]
    assert ((a >= 0) & (b >= 0) & (a != b)).sum() > 0


class _NoXY(SR.Restatement):
    """FLAWED: X x Y left out -- only the pairs with the rest of the contig are re-priced."""

    def groups(self, X, Y, R_):
        return [(X, R_), (Y, R_)]


class _YStays(SR.Restatement):
    """FLAWED: Y's shift forgotten -- X moves up, Y keeps its starts."""

    def new_layout(self, state, f, m_, l):
        S = SR.swap_layout(state, f, m_, l)
        m, sx, sy = SR._members(state, f, m_, l)
        S["start_bp"][m[sy]] = np.asarray(state["start_bp"])[m[sy]]
        return S


def test_flawed_restatements_miss_the_true_value():
    P = window_cases.small("w3")
    s = P["S_o_A_frags"]
    m = max(LR.contigs_of(s).values(), key=len)
    first, mid, last = np.array([m[20]]), np.array([m[22]]), np.array([m[26]])
    good = SR.restatement(P).swaps(s, first, mid, last)
    assert np.array_equal(SR.window(P).swaps(s, first, mid, last)[0], good[0])
    for cls in (_NoXY, _YStays):
        got = SR.restatement(P, cls=cls).swaps(s, first, mid, last)
        assert abs(int(got[0][0]) - int(good[0][0])) > 1e-9 * good[3][0] + 1, cls.__name__


# ---- graal_amd.swaps' host logic ---------------------------------------------------------------------------------------------------

def test_tilings_cover_every_adjacent_pair_once():
    s = _toy()                                                        # contig 0: 0..9, contig 1: 10..14, a ring 15..18
    sets = list(swaps.tilings(s, None, 4))
    seen = {}
    for i, (first, mid, last) in enumerate(sets):
        used = set()
        for f, m, l in zip(first, mid, last):
            assert f <= m < l
            frs = set(range(int(f), int(l) + 1))
            assert not (used & frs)                                   # disjoint within a set
            used |= frs
            assert (int(f), int(m), int(l)) not in seen
            seen[(int(f), int(m), int(l))] = i
    want = {(a, a + x - 1, a + w - 1) for lo, hi in ((0, 10), (10, 15)) for w in range(2, 5) for x in range(1, w) for a in range(lo, hi - w + 1)}
    assert set(seen) == want                                          # every pair of adjacent runs of <= 4 fragments together, no ring
    assert len(sets) == 2 * 1 + 3 * 2 + 4 * 3
    assert (10, 11, 14) in {(int(f), int(m), int(l)) for a in swaps.tilings(s, None, 5) for f, m, l in zip(*a)}   # a whole contig is kept
    big = LR.layout(np.full(40, 100), [[(f, 1) for f in range(40)]])
    assert len(list(swaps.tilings(big, None, 8))) == 168


def test_tilings_over_marks_use_units():
    s = _toy()
    marks = np.zeros(19, bool)
    marks[[2, 6, 11]] = True                                          # units: 0-2, 3-6, 7-9 | 10-11, 12-14
    got = [sorted(zip(f.tolist(), m.tolist(), l.tolist())) for f, m, l in swaps.tilings(s, marks, 3)]
    assert got == [[(0, 2, 6), (10, 11, 14)], [(3, 6, 9)], [(0, 2, 9)], [(0, 6, 9)]]


def test_plan_swaps_order_reach_and_ties():
    s = _toy()                                                        # 100 bp fragments: a span (f, l) covers [100 f, 100 (l + 1))
    V = swaps.SWAP_VALID
    cands = [(np.array([1, 4, 12]), np.array([1, 4, 12]), np.array([2, 5, 13]), np.array([5.0, 9.0, 9.0]), np.array([V, V, V], np.uint8)),
             (np.array([7, 8, 0]), np.array([7, 8, 0]), np.array([8, 9, 1]), np.array([3.0, 3.0, 50.0]), np.array([V, V, 2], np.uint8))]
    f, m, l, sc = swaps.plan_swaps(cands, s, reach_bp=150, min_score=1.0)
    # 9.0 twice: the lower (first, mid, last) first; (1, 2) lies 100 bp from (4, 5): dropped; (7, 8) ends 100 bp... starts 100 bp behind
    # (4, 5): dropped; (8, 9) 200 bp: stays; the NONFINITE 50.0 never
    assert list(zip(f.tolist(), m.tolist(), l.tolist())) == [(4, 4, 5), (12, 12, 13), (8, 8, 9)] and sc.tolist() == [9.0, 9.0, 3.0]
    f, m, l, sc = swaps.plan_swaps(cands, s, reach_bp=50, min_score=1.0)
    assert list(zip(f.tolist(), l.tolist())) == [(4, 5), (12, 13), (1, 2), (7, 8)]   # (8, 9) overlaps (7, 8), which comes first on the tie
    assert len(swaps.plan_swaps(cands, s, reach_bp=50, min_score=9.0)[0]) == 0
    assert len(swaps.plan_swaps(cands[0], s, reach_bp=0, min_score=0.0)[0]) == 3   # (a single tuple)


@pytest.mark.parametrize("spans", [[(0, 0, 2)], [(7, 8, 9)], [(1, 1, 2), (5, 6, 7)], [(1, 2, 3), (4, 4, 6)], [(0, 4, 9)], [(0, 0, 1), (2, 2, 3), (8, 8, 9)],
                                   [(0, 1, 3), (4, 8, 9)], [(11, 11, 12), (2, 3, 5)], [(10, 12, 14)]])
def test_swap_edit_writes_the_swapped_layout(spans):
    """swap_edit's cuts and joins through the edit restatement = swap_layout of the same swaps applied together, or that layout with
    the whole contig reversed (the edit's canonical chain order): a span at a head, at a tail, two with a gap, two adjacent, a whole
    contig, adjacent one-fragment pairs, two spans that tile the contig, spans in two contigs."""
    from tests import flip_reference as FR
    lens = np.arange(19) * 10 + 50
    s = LR.layout(lens, [[(f, 1 if f % 3 else -1) for f in range(10)], [(f, 1) for f in range(10, 15)], [(f, 1) for f in range(15, 19)]],
                  circular={2})
    first, mid, last = (np.array(x) for x in zip(*spans))
    cuts, joins = swaps.swap_edit(s, first, mid, last)
    used = joins.reshape(-1).tolist()
    assert len(used) == len(set(used))                                # a matching
    got, status = ER.edit(s, cuts, joins)
    assert got is not None, status
    want = SR.swap_layout(s, first, mid, last)
    assert not FR.same_layout(want, s)
    for c in {int(np.asarray(s["id_c"])[f]) for f in first}:
        sel = np.asarray(s["id_c"]) == c
        assert (np.asarray(got["id_c"])[sel] == c).all()
        alt = FR.reverse_contig(want, c)
        ok = [all(np.array_equal(np.asarray(got[k])[sel], np.asarray(w[k])[sel]) for k in LR.FIELDS) for w in (want, alt)]
        assert any(ok), spans
    rest = ~np.isin(np.asarray(s["id_c"]), [int(np.asarray(s["id_c"])[f]) for f in first])
    for k in LR.FIELDS:
        assert np.array_equal(np.asarray(got[k])[rest], np.asarray(s[k])[rest]), k


def test_swapping_back_is_the_identity():
    from tests import flip_reference as FR
    P = LR.case("sub3")
    s = P["S_o_A_frags"]
    first, mid, last = list(swaps.tilings(s, None, 3))[2]             # (1 fragment, 2 fragments)
    once = SR.swap_layout(s, first, mid, last)
    back = SR.swap_layout(once, *SR.swapped_back(s, first, mid, last))
    for k in LR.FIELDS:
        assert np.array_equal(np.asarray(back[k]), np.asarray(s[k])), k
    assert not FR.same_layout(once, s)


class _RestatedSwapEngine(_RestatedEngine):
    """The Engine calls swap_rounds makes, answered by the restatements: no device."""

    def __init__(self, P, state):
        super().__init__(P, state)
        self.WS = SR.window(P)

    def block_swaps(self, first, mid, last):
        q, c, st, _ = self.WS.swaps(self.state, first, mid, last)
        return np.where(st == SR.VALID, q / LR.Q, np.nan), c, st


def numpy_genome():
    """The scaffold tests' genome (1,000 bins, chromosomes of 400 / 300 / 200 / 100) with contacts drawn by numpy (Poisson of
    tests/sim_reference.pair_lambda, seed 5): test_flips_cpu's."""
    from graal_amd import synth
    from tests import sim_reference as SIM
    par = synth.make_param_simu(fact=1500.0, v_inter=0.5)
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(4, 3, 2, 1), param=par)
    s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
    a, b = np.triu_indices(1000, 1)
    lam = SIM.pair_lambda(SIM.sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], s), a, b,
                          P["mean_squared_frags_per_bin"], par)
    v = np.random.RandomState(5).poisson(np.maximum(lam, 0))
    k = v > 0
    P["coo_row"], P["coo_col"], P["coo_val"], P["param_simu"] = a[k].astype(np.int32), b[k].astype(np.int32), v[k].astype(np.int32), par
    return P, s


def test_swap_rounds_over_the_restatement_restore_planted_transpositions():
    """The scaffold tests' genome with contacts drawn by numpy (seed 5) and the seven transpositions of tests/swap_reference.PLANTS.
    As the windowed restatement gives them: in the true layout the largest of the 27,440 swaps of the complete tilings up to 8
    fragments (168 sets) scores 2.09; swapped back, the planted swaps gain 98.8, 1,033.1, 2,268.9, 3,189.5, 712.1, 2,228.7 and 402.9.
    min_score = 20 lies between; swap_rounds(min_score=20) driven by the restatements restores every chromosome's true order, every
    kept round raises logL, and the planted layout fails the check of the order."""
    P, s = numpy_genome()
    W = SR.window(P)
    spurious, n = -np.inf, 0
    for first, mid, last in swaps.tilings(s, None, 8):
        q = W.swaps(s, first, mid, last)[0]
        spurious = max(spurious, q.max() / LR.Q); n += len(q)
    bad, first, mid, last = SR.planted(s)
    gains = W.swaps(bad, first, mid, last)[0] / LR.Q
    print("swaps scored %d, largest spurious %.2f, planted gains %s" % (n, spurious, np.round(gains, 1).tolist()))
    assert spurious < 20.0 < gains.min(), (spurious, gains)
    with pytest.raises(AssertionError):
        SR.assert_true_chromosomes(bad, s)
    e = _RestatedSwapEngine(P, bad)
    rec = swaps.swap_rounds(e, max_frags=8, junction_below=0.0, max_units=3, min_score=20.0)
    kept = [r["logL"] for r in rec if r["kept"]]
    assert len(kept) >= 2 and all(b > a for a, b in zip(kept, kept[1:])), rec
    SR.assert_true_chromosomes(e.download_frags(), s)


def test_tsv_writers(tmp_path):
    rec = [{"round": 0, "swaps": 0, "contigs": 4, "logL": -1.5, "kept": 1}, {"round": 1, "swaps": 3, "contigs": 4, "logL": -1.25, "kept": 1}]
    assert swaps.write_swap_rounds_tsv(str(tmp_path / "swap.tsv"), rec) == 2
    lines = (tmp_path / "swap.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(swaps.ROUND_COLUMNS) and lines[2].split("\t") == ["1", "3", "4", "-1.25", "1"]
    t = {k: np.array([1, 2]) for k in swaps.COLUMNS}
    t["score"] = np.array([0.5, np.nan])
    assert swaps.write_swaps_tsv(str(tmp_path / "swaps.tsv"), t) == 2
    lines = (tmp_path / "swaps.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(swaps.COLUMNS) and lines[2].split("\t")[swaps.COLUMNS.index("score")] == "nan"


def test_block_swaps_refuse_without_gpu():
    """graal_block_swaps on a handle without a device: an error, nothing computed on the host, outputs untouched."""
    import ctypes
    from graal_amd import build as gbuild
    from graal_amd import lib
    gbuild.build_hip()
    L = lib.load()
    h = ctypes.c_void_p()
    if L.graal_create(0, ctypes.byref(h)) == 0:
        L.graal_destroy(h)
        pytest.skip("a GPU is present: tests/test_swaps_gpu.py covers the engine")
    try:
        a = np.zeros(1, np.int32); q = np.full(1, 7, np.int64); st = np.full(1, 9, np.uint8)
        rc = L.graal_block_swaps(h, 1, a.ctypes.data_as(lib._i32p), a.ctypes.data_as(lib._i32p), a.ctypes.data_as(lib._i32p),
                                 q.ctypes.data_as(lib._i64p), q.ctypes.data_as(lib._i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        assert rc != 0 and L.graal_last_error(h).decode() and q[0] == 7 and st[0] == 9
    finally:
        L.graal_destroy(h)
