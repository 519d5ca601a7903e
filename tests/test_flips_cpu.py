"""graal_block_flips' numpy restatements against a dense likelihood and against each other, a flawed restatement that must miss, and
graal_amd.flips' host logic (tilings, marks, plan, edit) on hand-built cases.  No GPU."""
import numpy as np
import pytest

from graal_amd import flips
from tests import edit_reference as ER
from tests import flip_reference as FR
from tests import link_reference as LR
from tests import window_cases
from tests.sim_reference import sub_records


def _tiling_blocks(s, max_units=4, marks=None):
    sets = list(flips.tilings(s, marks, max_units))
    return sets


def _extras(s):
    """One whole-contig block of a linear contig and, where the layout holds a ring, a block inside it."""
    out = []
    circ = np.asarray(s["circ"])
    lists = LR.contigs_of(s)
    lin = [m for m in lists.values() if circ[m[0]] == 0 and len(m) > 1]
    ring = [m for m in lists.values() if circ[m[0]] == 1 and len(m) > 2]
    out.append((lin[0][0], lin[0][-1]))
    if ring:
        out.append((ring[0][1], ring[0][2]))
    return np.array([a for a, _ in out]), np.array([b for _, b in out])


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("sub1", True)])
def test_brute_force_equals_dense_difference(name, quirk):
    """F = the difference of a dense sum over EVERY sub-fragment pair between the flipped layout, its pairs inside the block and inside
    the rest of the contig priced with their old centres, and the current layout (links' tolerance), for every block of the tilings
    m <= 4.  The dense sum has no notion of which pairs a flip changes: the mirrored mixed bins against the other contigs are in it."""
    P = LR.case(name)
    s = P["S_o_A_frags"]
    R = FR.restatement(P, quirk=quirk)
    centre = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], s)[0]
    base = LR.dense_loglik(R, s, LR.pricer(R, s, centre))
    idc = np.asarray(s["id_c"])
    n_blocks = 0
    for first, last in _tiling_blocks(s):
        q, c, st, A = R.flips(s, first, last)
        assert (st == FR.VALID).all()
        for k in range(len(first)):
            F = FR.flip_layout(s, first[k], last[k])
            cF = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], F)[0]
            m, sl = FR._members(s, int(first[k]), int(last[k]))
            in_b = np.zeros(R.n, bool); in_b[m[sl]] = True
            in_r = (idc == idc[first[k]]) & ~in_b
            fixed = [(in_b[R.bin_of], centre), (in_r[R.bin_of], centre)]
            d = LR.dense_loglik(R, F, LR.pricer(R, F, cF, fixed)) - base
            assert abs(q[k] / LR.Q - d) <= 1e-7 * A[k] / LR.Q + 1e-6, (first[k], last[k], q[k] / LR.Q, d)
            n_blocks += 1
    assert n_blocks >= 100


def test_brute_force_statuses_whole_and_circular():
    P = LR.case("circ")
    s = P["S_o_A_frags"]
    first, last = _extras(s)
    q, c, st, A = FR.restatement(P).flips(s, first, last)
    assert st.tolist() == [FR.WHOLE, FR.CIRCULAR] and not q.any() and not c.any()
    q, c, st, A = FR.window(P).flips(s, first, last)
    assert st.tolist() == [FR.WHOLE, FR.CIRCULAR] and not q.any() and not c.any()


def _seventh_marks(s):
    marks = np.zeros(len(s["id_c"]), bool)
    nx = np.asarray(s["next"])
    marks[np.nonzero(nx >= 0)[0][::7]] = True
    return marks


@pytest.mark.parametrize("name,quirk", [("w1", False), ("w1", True), ("w3", False), ("w3", True)])
def test_windowed_equals_brute_force(name, quirk):
    P = window_cases.small(name)
    s = P["S_o_A_frags"]
    B, W = FR.restatement(P, quirk=quirk), FR.window(P, quirk=quirk)
    sets = _tiling_blocks(s) + _tiling_blocks(s, 3, _seventh_marks(s))
    assert len(sets) == 10 + 6
    far = 0
    for first, last in sets:
        got, want = W.flips(s, first, last), B.flips(s, first, last)
        for g, w, what in zip(got, want, ("q", "contacts", "status", "A")):
            assert np.array_equal(g, w), (what, np.nonzero(g != w)[0][:5])
        span = (np.asarray(s["start_bp"])[last] + np.asarray(s["len_bp"])[last] - np.asarray(s["start_bp"])[first]).astype(np.int64)
        far += int((span > 2 * W.reach + 2000).sum())
    assert far > 0                                # (blocks longer than two windows: their interior does not contribute)


def test_windowed_equals_brute_force_in_one_call_with_neighbouring_blocks():
    """Blocks of one call less than a window apart, with contacts between them: each carries its own term (only that block flipped)."""
    P = window_cases.small("w3")
    s = P["S_o_A_frags"]
    first, last = next(iter(flips.tilings(s, None, 3)))
    got, want = FR.window(P, quirk=True).flips(s, first, last), FR.restatement(P, quirk=True).flips(s, first, last)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert (got[1] > 0).sum() > 10


class _OldWalk(FR.Restatement):
    """FLAWED: the flip mirrors the positions but every bin keeps walking its sub-fragments in its old orientation."""

    def new_centres(self, flipped):
        f = dict(flipped)
        f["ori"] = self._ori_before
        return sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, f)[0]


class _LeftFlankOnly(FR.Window):
    one_flank = True


def test_a_flawed_restatement_misses_the_true_value():
    """Both flaws move the score of blocks built to show them: a block of three-sub-fragment bins (the walk), a block with fragments on
    both sides (the right flank's mass)."""
    P = window_cases.small("w3")
    s = P["S_o_A_frags"]
    m = max(LR.contigs_of(s).values(), key=len)
    first, last = np.array([m[20]]), np.array([m[23]])
    good = FR.restatement(P).flips(s, first, last)
    bad = FR.restatement(P, cls=_OldWalk)
    bad._ori_before = np.asarray(s["ori"]).copy()
    got = bad.flips(s, first, last)
    assert abs(int(got[0][0]) - int(good[0][0])) > 1e-9 * good[3][0] + 1
    W = FR.window(P).flips(s, first, last)
    assert np.array_equal(W[0], good[0])
    got = FR.window(P, cls=_LeftFlankOnly).flips(s, first, last)
    assert abs(int(got[0][0]) - int(good[0][0])) > 1e-9 * good[3][0] + 1


# ---- graal_amd.flips' host logic ---------------------------------------------------------------------------------------------------

def _toy():
    """Contig 0: fragments 0..9 forward; contig 1: 10..14; contig 2: a ring 15..18; 100 bp each."""
    lens = np.full(19, 100)
    return LR.layout(lens, [[(f, 1) for f in range(10)], [(f, 1) for f in range(10, 15)], [(f, 1) for f in range(15, 19)]], circular={2})


def test_tilings_cover_every_short_run_once():
    s = _toy()
    sets = list(flips.tilings(s, None, 4))
    seen = {}
    for i, (first, last) in enumerate(sets):
        used = set()
        for f, l in zip(first, last):
            frs = set(range(int(f), int(l) + 1))
            assert not (used & frs)                                   # disjoint within a set
            used |= frs
            assert (int(f), int(l)) not in seen
            seen[(int(f), int(l))] = i
    want = {(a, a + m - 1) for lo, hi in ((0, 10), (10, 15)) for m in range(1, 5) for a in range(lo, hi - m + 1)}
    assert set(seen) == want                                          # every run of <= 4 fragments of a linear contig, no ring, no whole
    assert len(sets) == 10
    assert not any(k == (0, 9) or k == (10, 14) for k in set(seen) | {(f, l) for f, l in flips.tilings(s, None, 10) for f, l in zip(f, l)})


def test_tilings_over_marks_use_units():
    s = _toy()
    marks = np.zeros(19, bool)
    marks[[2, 6, 11]] = True                                          # units: 0-2, 3-6, 7-9 | 10-11, 12-14
    got = [sorted(zip(f.tolist(), l.tolist())) for f, l in flips.tilings(s, marks, 2)]
    assert got == [[(0, 2), (3, 6), (7, 9), (10, 11), (12, 14)], [(0, 6)], [(3, 9)]]


def test_joined_marks_mark_new_neighbours_only():
    before = LR.layout(np.full(8, 100), [[(0, 1), (1, 1), (2, 1)], [(3, 1), (4, -1)], [(5, 1), (6, 1), (7, 1)]])
    # contig 1 reversed and appended to contig 0; inside contig 2 fragment 6 turned round
    now = LR.layout(np.full(8, 100), [[(0, 1), (1, 1), (2, 1), (4, 1), (3, -1)], [(5, 1), (6, -1), (7, 1)]])
    marks = flips.joined_marks(before, now)
    assert np.nonzero(marks)[0].tolist() == [2, 5, 6]
    assert not flips.joined_marks(now, now).any()


def test_plan_flips_order_reach_and_ties():
    s = _toy()                                                        # 100 bp fragments: block (f, l) covers [100 f, 100 (l + 1))
    V = flips.FLIP_VALID
    cands = [(np.array([1, 4, 12]), np.array([2, 5, 13]), np.array([5.0, 9.0, 9.0]), np.array([V, V, V], np.uint8)),
             (np.array([7, 8, 0, 3]), np.array([7, 9, 0, 3]), np.array([3.0, 3.0, 50.0, np.nan]), np.array([V, V, 3, 3], np.uint8))]
    f, l, sc = flips.plan_flips(cands, s, reach_bp=150, min_score=1.0)
    # 9.0 twice: the lower (first, last) first; (1, 2) lies 100 bp from (4, 5): dropped; (7, 7) is 100 bp away, (8, 9) 200 bp: (8, 9) stays
    assert list(zip(f.tolist(), l.tolist())) == [(4, 5), (12, 13), (8, 9)] and sc.tolist() == [9.0, 9.0, 3.0]
    f, l, sc = flips.plan_flips(cands, s, reach_bp=50, min_score=1.0)
    assert list(zip(f.tolist(), l.tolist())) == [(4, 5), (12, 13), (1, 2), (7, 7)]   # (8, 9) touches (7, 7), which comes first on the tie
    f, l, sc = flips.plan_flips(cands, s, reach_bp=50, min_score=9.0)
    assert len(f) == 0
    f, l, sc = flips.plan_flips(cands[0], s, reach_bp=0, min_score=0.0)   # (a single tuple)
    assert len(f) == 3


@pytest.mark.parametrize("blocks", [[(0, 2)], [(7, 9)], [(1, 2), (5, 7)], [(1, 3), (4, 6)], [(4, 4)], [(0, 0), (1, 1), (9, 9)],
                                    [(0, 3), (4, 9)], [(11, 12), (2, 5)]])
def test_flip_edit_writes_the_flipped_layout(blocks):
    """flip_edit's cuts and joins through the edit restatement = flip_layout of the same blocks applied together, or that layout with
    the whole contig reversed (the edit's canonical chain order): a block at a head, at a tail, two with a gap, two adjacent, one
    fragment, adjacent single fragments, two blocks that tile the contig, blocks in two contigs."""
    lens = np.arange(19) * 10 + 50
    s = LR.layout(lens, [[(f, 1 if f % 3 else -1) for f in range(10)], [(f, 1) for f in range(10, 15)], [(f, 1) for f in range(15, 19)]],
                  circular={2})
    first, last = np.array([a for a, _ in blocks]), np.array([b for _, b in blocks])
    cuts, joins = flips.flip_edit(s, first, last)
    used = joins.reshape(-1).tolist()
    assert len(used) == len(set(used))                                # a matching
    got, status = ER.edit(s, cuts, joins)
    assert got is not None, status
    want = FR.flip_layout(s, first, last)
    for c in {int(np.asarray(s["id_c"])[f]) for f in first}:
        sel = np.asarray(s["id_c"]) == c
        assert (np.asarray(got["id_c"])[sel] == c).all()
        alt = FR.reverse_contig(want, c)
        ok = [all(np.array_equal(np.asarray(got[k])[sel], np.asarray(w[k])[sel]) for k in LR.FIELDS) for w in (want, alt)]
        assert any(ok), blocks
    rest = ~np.isin(np.asarray(s["id_c"]), [int(np.asarray(s["id_c"])[f]) for f in first])
    for k in LR.FIELDS:
        assert np.array_equal(np.asarray(got[k])[rest], np.asarray(s[k])[rest]), k


def test_flip_layout_twice_is_the_identity():
    P = LR.case("sub3")
    s = P["S_o_A_frags"]
    first, last = next(iter(flips.tilings(s, None, 3)))
    once = FR.flip_layout(s, first, last)
    back = FR.flip_layout(once, last, first)
    for k in LR.FIELDS:
        assert np.array_equal(np.asarray(back[k]), np.asarray(s[k])), k
    assert not FR.same_layout(once, s)


class _RestatedEngine(flips._sc.Engine):
    """The Engine calls flip_rounds makes, answered by the restatements: no device."""

    def __init__(self, P, state):
        from oracle.sparse_numpy import SparseScorer
        self.W = FR.window(P)
        self.sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                               P["mean_squared_frags_per_bin"], P["param_simu"])
        self.param = np.asarray(P["param_simu"], np.float32)
        self._h = None
        self.upload_frags(state)

    def upload_frags(self, soa):
        self.state = {k: np.array(v, np.int32) for k, v in soa.items()}
        self.n = len(self.state["id_c"])

    def download_frags(self, out=None):
        return {k: v.copy() for k, v in self.state.items()}

    def relabel_contigs(self):
        return 0

    def eval_full(self):
        return self.sp.full(self.state, windowed=True)

    def junction_scores(self):
        J, st, _ = self.W.junction_scores(self.state)
        return np.where(st == 0, J / LR.Q, np.nan), st

    def block_flips(self, first, last):
        q, c, st, _ = self.W.flips(self.state, first, last)
        return np.where(st == FR.VALID, q / LR.Q, np.nan), c, st

    def edit_layout(self, cuts=(), joins=()):
        got, status = ER.edit(self.state, cuts, joins)
        assert got is not None, status
        self.upload_frags(got)
        return status


def test_flip_rounds_over_the_restatement_restore_planted_inversions():
    """The scaffold tests' genome with contacts drawn by numpy (Poisson of tests/sim_reference.pair_lambda, seed 5) and the seven
    inversions of tests/flip_reference.PLANTS: in the true layout 4 of the 6,888 runs of 2-8 fragments score above 0, the largest 2.1;
    the planted blocks gain 372.8 to 7,660.8; flip_rounds(min_score=20) driven by the restatements flips all seven back in one round."""
    from graal_amd import synth
    from tests import sim_reference as SR
    par = synth.make_param_simu(fact=1500.0, v_inter=0.5)
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(4, 3, 2, 1), param=par)
    s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
    a, b = np.triu_indices(1000, 1)
    lam = SR.pair_lambda(SR.sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], s), a, b,
                         P["mean_squared_frags_per_bin"], par)
    v = np.random.RandomState(5).poisson(np.maximum(lam, 0))
    k = v > 0
    P["coo_row"], P["coo_col"], P["coo_val"], P["param_simu"] = a[k].astype(np.int32), b[k].astype(np.int32), v[k].astype(np.int32), par
    W = FR.window(P)
    spurious = []
    for first, last in flips.tilings(s, None, 8):
        q = W.flips(s, first, last)[0][first != last]
        spurious.append(q.max() / LR.Q if len(q) else -np.inf)
    assert 0 < max(spurious) < 3
    bad, first, last = FR.planted(s)
    gains = W.flips(bad, last, first)[0] / LR.Q                      # (in the planted layout a block starts at its old last fragment)
    assert gains.min() > 300 and abs(gains.min() - 372.8) < 0.1
    e = _RestatedEngine(P, bad)
    rec = flips.flip_rounds(e, max_frags=8, junction_below=0.0, max_units=3, min_score=20.0)
    assert [r["flips"] for r in rec] == [0, 7] and rec[1]["kept"] == 1 and rec[1]["logL"] > rec[0]["logL"]
    FR.assert_true_chromosomes_and_orientations(e.download_frags(), s)
    with pytest.raises(AssertionError):
        FR.assert_true_chromosomes_and_orientations(bad, s)


def test_tsv_writers(tmp_path):
    rec = [{"round": 0, "flips": 0, "contigs": 4, "logL": -1.5, "kept": 1}, {"round": 1, "flips": 3, "contigs": 4, "logL": -1.25, "kept": 1}]
    assert flips.write_flip_rounds_tsv(str(tmp_path / "flip.tsv"), rec) == 2
    lines = (tmp_path / "flip.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(flips.ROUND_COLUMNS) and lines[2].split("\t") == ["1", "3", "4", "-1.25", "1"]
    t = {k: np.array([1, 2]) for k in flips.COLUMNS}
    t["score"] = np.array([0.5, np.nan])
    assert flips.write_flips_tsv(str(tmp_path / "flips.tsv"), t) == 2
    lines = (tmp_path / "flips.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(flips.COLUMNS) and lines[2].split("\t")[6] == "nan"


def test_block_flips_refuse_without_gpu():
    """graal_block_flips on a handle without a device: an error, nothing computed on the host, outputs untouched."""
    import ctypes
    from graal_amd import build as gbuild
    from graal_amd import lib
    gbuild.build_hip()
    L = lib.load()
    h = ctypes.c_void_p()
    if L.graal_create(0, ctypes.byref(h)) == 0:
        L.graal_destroy(h)
        pytest.skip("a GPU is present: tests/test_flips_gpu.py covers the engine")
    try:
        a = np.zeros(1, np.int32); q = np.full(1, 7, np.int64); st = np.full(1, 9, np.uint8)
        rc = L.graal_block_flips(h, 1, a.ctypes.data_as(lib._i32p), a.ctypes.data_as(lib._i32p), q.ctypes.data_as(lib._i64p),
                                 q.ctypes.data_as(lib._i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        assert rc != 0 and L.graal_last_error(h).decode() and q[0] == 7 and st[0] == 9
    finally:
        L.graal_destroy(h)
