"""graal_block_excisions' numpy restatements against a dense likelihood, against each other, against the junction restatement (a span
at a head or a tail is a plain cut) and against the insertion restatement (an excision is the inverse of an insertion); span_check.h's
third kind; and graal_amd.excise's host logic (tilings, plan, edit, writers) on hand-built cases.  No GPU."""
import ctypes

import numpy as np
import pytest

from graal_amd import excise
from graal_amd.lib import EXCISE_CIRCULAR, EXCISE_VALID, EXCISE_WHOLE
from tests import edit_reference as ER
from tests import excise_reference as XR
from tests import link_reference as LR
from tests import test_span_check_cpu as SC
from tests import util, window_cases
from tests.sim_reference import sub_records


def long_runs(s, lengths=(10, 17, 30)):
    """(first, last) of one run of each length in every linear contig that holds it twice over, apart from each other."""
    first, last = [], []
    circ = np.asarray(s["circ"])
    for m in LR.contigs_of(s).values():
        at = 2
        for w in lengths:
            if circ[m[0]] == 0 and at + w + 2 < len(m):
                first.append(m[at]); last.append(m[at + w - 1])
                at += w + 3
    return np.array(first, np.int32), np.array(last, np.int32)


def _problem(name):
    return window_cases.small_cut(name[:2]) if name.endswith("_cut") else window_cases.small(name)


@pytest.mark.parametrize("name,quirk", [(n, q) for n in ("w1", "w3", "w1_cut", "w3_cut") for q in (False, True)])
def test_windowed_equals_brute_force(name, quirk):
    """Every tiling up to 3 fragments (spans of one call less than a window apart, with contacts between them: each is scored alone)
    and runs of 10, 17 and 30 fragments: the same q, contacts, status and sum of |terms|."""
    P = _problem(name)
    s = P["S_o_A_frags"]
    B, W = XR.restatement(P, quirk=quirk), XR.window(P, quirk=quirk)
    sets = list(excise.tilings(s, None, 3)) + [long_runs(s)]
    assert len(sets) == 7
    n, closing, far = 0, 0, 0
    for first, last in sets:
        parts = {}
        got, want = W.excisions(s, first, last, parts), B.excisions(s, first, last)
        for g, w, what in zip(got, want, ("q", "contacts", "status", "A")):
            assert np.array_equal(g, w), (what, np.nonzero(g != w)[0][:5])
        n += len(first); closing += int(parts["closing_fed"].sum()); far += int((parts["far"] != 0).sum())
    assert n > 300 and closing > 100
    if quirk and name.startswith("w3"):
        assert far > 0                            # (the pairs beyond the window that the indexing prices apart)


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("sub1", True)])
def test_brute_force_equals_dense_difference(name, quirk):
    """E = the difference of a dense sum over EVERY sub-fragment pair between the excised layout, its pairs inside X, inside L and
    inside R priced with their old centres, and the current layout (the flips' tolerance), for every span of the tilings m <= 4.  The
    dense sum has no notion of which pairs an excision changes."""
    P = LR.case(name)
    s = P["S_o_A_frags"]
    R = XR.restatement(P, quirk=quirk)
    centre = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], s)[0]
    base = LR.dense_loglik(R, s, LR.pricer(R, s, centre))
    n_spans = 0
    for first, last in excise.tilings(s, None, 4):
        q, c, st, A = R.excisions(s, first, last)
        assert (st == XR.VALID).all()
        for k in range(len(first)):
            S = XR.excise_layout(s, first[k], last[k])
            cS = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], S)[0]
            m, sl = XR._members(s, int(first[k]), int(last[k]))
            fixed = []
            for g in (m[sl], m[:sl.start], m[sl.stop:]):
                mask = np.zeros(R.n, bool); mask[g] = True
                fixed.append((mask[R.bin_of], centre))
            d = LR.dense_loglik(R, S, LR.pricer(R, S, cS, fixed)) - base
            assert abs(q[k] / LR.Q - d) <= 1e-7 * A[k] / LR.Q + 1e-6, (first[k], last[k], q[k] / LR.Q, d)
            n_spans += 1
    assert n_spans >= 100


def test_statuses_whole_and_circular():
    P = LR.case("circ")
    s = P["S_o_A_frags"]
    circ = np.asarray(s["circ"])
    lists = LR.contigs_of(s)
    lin = [m for m in lists.values() if circ[m[0]] == 0 and len(m) > 1][0]
    ring = [m for m in lists.values() if circ[m[0]] == 1 and len(m) > 2][0]
    first, last = np.array([lin[0], ring[1]]), np.array([lin[-1], ring[2]])
    for R in (XR.restatement(P), XR.window(P)):
        q, c, st, A = R.excisions(s, first, last)
        assert st.tolist() == [XR.WHOLE, XR.CIRCULAR] and not q.any() and not c.any()
    assert (XR.VALID, XR.WHOLE, XR.CIRCULAR) == (EXCISE_VALID, EXCISE_WHOLE, EXCISE_CIRCULAR)


@pytest.mark.parametrize("name,quirk", [("w1", False), ("w3", False), ("w3", True)])
def test_a_head_or_tail_span_is_a_plain_cut(name, quirk):
    """L or R empty: E = -(J of the junction restatement at the one junction the excision cuts), to 1e-9 A + 1 (the junction sums a
    pair with its lower position outer, the excision with X's fragment outer)."""
    P = window_cases.small(name)
    s = P["S_o_A_frags"]
    W = XR.window(P, quirk=quirk)
    first, last, junc = [], [], []
    for m in LR.contigs_of(s).values():
        for w in (1, 2, 9, 30):
            first += [m[0], m[-w]]; last += [m[w - 1], m[-1]]; junc += [m[w - 1], m[-w - 1]]
    first, last = np.array(first), np.array(last)
    J = W.junction_direct(s, junc)
    for k in range(len(first)):                  # (one span per call: head and tail spans of a contig may overlap)
        q, c, st, A = W.excisions(s, first[k:k + 1], last[k:k + 1])
        j, bad, _ = J[int(junc[k])]
        assert st[0] == XR.VALID and not bad
        assert abs(int(q[0]) + int(j)) <= 1e-9 * A[0] + 1, (k, int(q[0]), int(j))
        assert q[0] != 0


@pytest.mark.parametrize("name,quirk", [("w1", False), ("w3", False), ("w3", True)])
def test_an_excision_is_the_inverse_of_an_insertion(name, quirk):
    """E = -(the windowed insertion score of X into the junction L.tail | R.head, rev 0) computed on the excised layout."""
    P = window_cases.small(name)
    s = P["S_o_A_frags"]
    W = XR.window(P, quirk=quirk)
    n = 0
    for first, last in list(excise.tilings(s, None, 3))[::2] + [long_runs(s)]:
        q, c, st, A = W.excisions(s, first, last)
        pos, prev, nxt = (np.asarray(s[k]) for k in ("pos", "prev", "next"))
        for k in np.nonzero((prev[first] >= 0) & (nxt[last] >= 0))[0][::5]:
            S = XR.excise_layout(s, first[k], last[k])
            iq, ist, iA = W.insertion_scores(S, [first[k]], [prev[first[k]]], [0])
            assert st[k] == XR.VALID and ist[0] == 0
            assert abs(int(q[k]) + int(iq[0])) <= 1e-9 * A[k] + 1, (first[k], last[k], int(q[k]), int(iq[0]))
            n += 1
    assert n >= 40


# ---- span_check.h, kind 2 ----------------------------------------------------------------------------------------------------------

def _restated(rows):
    """tests/test_span_check_cpu.restated for the third kind: no mid, a whole contig set aside."""
    for k, (sf, sm, sl, lf, lm, ll) in enumerate(rows[:, :6].tolist()):
        if sf < 0:
            return k, SC.NO_SLOT
        if lf != lm or lf != ll:
            return k, SC.TWO_CONTIGS
        if sf > sm:
            return k, SC.MID_BEFORE_FIRST
        if any(not (sl < f2 or l2 < sf) for f2, l2 in rows[:k, [0, 2]].tolist()):
            return k, SC.OVERLAP
    st, scored = [], []
    for k, r in enumerate(rows.tolist()):
        if r[11]:
            st.append(EXCISE_CIRCULAR)
        elif r[0] == r[9] and r[2] == r[9] + r[10] - 1:
            st.append(EXCISE_WHOLE)
        else:
            st.append(EXCISE_VALID)
            scored.append(k)
    return None, st, sorted(scored, key=lambda k: rows[k, 0])


def test_span_check_of_excisions_equals_the_restatement():
    """Every refusal reason, WHOLE, CIRCULAR and the order of the scored records, on seeded span lists."""
    L = util.hostcheck()
    L.hc_span_check.restype = ctypes.c_int
    i32p, u8p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
    L.hc_span_check.argtypes = [ctypes.c_int, ctypes.c_int, i32p, i32p, u8p, i32p]
    rs = np.random.RandomState(22)
    refused, statuses, accepted2 = [], [], 0
    for _ in range(3000):
        rows = SC.random_list(rs, False)
        nb = len(rows)
        out, st, ids = np.full(2, -7, np.int32), np.full(nb, 255, np.uint8), np.full(nb, -7, np.int32)
        m = L.hc_span_check(2, nb, rows.ctypes.data_as(i32p), out.ctypes.data_as(i32p), st.ctypes.data_as(u8p), ids.ctypes.data_as(i32p))
        want = _restated(rows)
        if want[0] is not None:
            assert m == -1 and (int(out[0]), int(out[1])) == want, rows
            assert (st == 255).all() and (ids == -7).all()
            refused.append(want[1])
        else:
            assert m == len(want[2]) and int(out[0]) == -1 and int(out[1]) == 0, rows
            assert st.tolist() == want[1] and ids[:m].tolist() == want[2], rows
            statuses += want[1]; accepted2 += len(want[2]) >= 2
    assert min(refused.count(w) for w in (SC.NO_SLOT, SC.TWO_CONTIGS, SC.MID_BEFORE_FIRST, SC.OVERLAP)) >= 20
    assert accepted2 >= 100 and min(statuses.count(x) for x in (EXCISE_VALID, EXCISE_WHOLE, EXCISE_CIRCULAR)) >= 20


# ---- graal_amd.excise's host logic -------------------------------------------------------------------------------------------------

def _toy():
    """Contig 0: fragments 0..9 forward; contig 1: 10..14; contig 2: a ring 15..18; 100 bp each."""
    lens = np.full(19, 100)
    return LR.layout(lens, [[(f, 1) for f in range(10)], [(f, 1) for f in range(10, 15)], [(f, 1) for f in range(15, 19)]], circular={2})


def test_tilings_cover_every_short_run_once():
    s = _toy()
    sets = list(excise.tilings(s, None, 4))
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
    assert set(seen) == want                                          # every run of <= 4 fragments of a linear contig, no ring
    assert len(sets) == 10
    assert len(list(excise.tilings(s))) == 6                          # (max_units defaults to 3)
    marks = np.zeros(19, bool)
    marks[[2, 6, 11]] = True                                          # units: 0-2, 3-6, 7-9 | 10-11, 12-14
    got = [sorted(zip(f.tolist(), l.tolist())) for f, l in excise.tilings(s, marks, 2)]
    assert got == [[(0, 2), (3, 6), (7, 9), (10, 11), (12, 14)], [(0, 6)], [(3, 9)]]
    one = LR.layout(np.full(3, 100), [[(0, 1)], [(1, 1), (2, 1)]])
    assert [list(zip(f.tolist(), l.tolist())) for f, l in excise.tilings(one, None, 3)] == [[(1, 1), (2, 2)]]   # a whole contig: nothing to cut


def test_plan_excisions_order_reach_and_ties():
    s = _toy()                                                        # 100 bp fragments: span (f, l) covers [100 f, 100 (l + 1))
    V = EXCISE_VALID
    cands = [(np.array([1, 4, 12]), np.array([2, 5, 13]), np.array([5.0, 9.0, 9.0]), np.array([V, V, V], np.uint8)),
             (np.array([7, 8, 0, 3]), np.array([7, 9, 0, 3]), np.array([3.0, 3.0, 50.0, np.nan]), np.array([V, V, 3, 3], np.uint8))]
    f, l, sc = excise.plan_excisions(cands, s, reach_bp=150, min_score=1.0)
    assert list(zip(f.tolist(), l.tolist())) == [(4, 5), (12, 13), (8, 9)] and sc.tolist() == [9.0, 9.0, 3.0]
    f, l, sc = excise.plan_excisions(cands, s, reach_bp=50, min_score=1.0)
    assert list(zip(f.tolist(), l.tolist())) == [(4, 5), (12, 13), (1, 2), (7, 7)]
    assert len(excise.plan_excisions(cands, s, reach_bp=50, min_score=9.0)[0]) == 0
    assert len(excise.plan_excisions(cands[0], s, reach_bp=0, min_score=0.0)[0]) == 3   # (a single tuple)


@pytest.mark.parametrize("spans", [[(0, 2)], [(7, 9)], [(1, 2), (5, 7)], [(1, 3), (4, 6)], [(4, 4)], [(0, 0), (1, 1), (9, 9)],
                                   [(0, 3), (4, 8)], [(11, 12), (2, 5)], [(3, 3), (5, 5), (7, 7)], [(6, 7), (1, 2)]])
def test_excise_edit_writes_the_excised_layout(spans):
    """excise_edit's cuts and joins through the edit restatement = excise_layout of the same spans applied together, up to labels and
    the reversal of whole contigs (the edit's canonical chain order): a span at a head, at a tail, two with a gap, two adjacent, one
    fragment, adjacent single fragments at both ends, two spans that leave one fragment, spans in two contigs, every other fragment."""
    lens = np.arange(19) * 10 + 50
    s = LR.layout(lens, [[(f, 1 if f % 3 else -1) for f in range(10)], [(f, 1) for f in range(10, 15)], [(f, 1) for f in range(15, 19)]],
                  circular={2})
    first, last = np.array([a for a, _ in spans]), np.array([b for _, b in spans])
    cuts, joins = excise.excise_edit(s, first, last)
    used = joins.reshape(-1).tolist()
    assert len(used) == len(set(used))                                # a matching
    got, status = ER.edit(s, cuts, joins)
    assert got is not None, status
    want = XR.excise_layout(s, first, last)
    assert XR.chains(got) == XR.chains(want)
    assert len(XR.chains(want)) == 3 + len(spans)
    for c, m in LR.contigs_of(want).items():                          # a contig the edit did not turn round has excise_layout's fields
        if np.array_equal(np.asarray(got["ori"])[m], np.asarray(want["ori"])[m]):
            for k in ("pos", "start_bp", "l_cont", "l_cont_bp", "prev", "next", "circ"):
                assert np.array_equal(np.asarray(got[k])[m], np.asarray(want[k])[m]), (c, k)
    with pytest.raises(ValueError):
        excise.excise_edit(s, np.array([1, 2]), np.array([3, 4]))


def test_tsv_writers(tmp_path):
    rec = [{"round": 0, "excisions": 0, "contigs": 4, "logL": -1.5, "kept": 1}, {"round": 1, "excisions": 3, "contigs": 7, "logL": -1.25, "kept": 1}]
    assert excise.write_excise_rounds_tsv(str(tmp_path / "excise.tsv"), rec) == 2
    lines = (tmp_path / "excise.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(excise.ROUND_COLUMNS) and lines[2].split("\t") == ["1", "3", "7", "-1.25", "1"]
    assert excise.COLUMNS == ("first", "last", "contig", "pos_first", "pos_last", "frags", "score", "contacts", "status")
    t = {k: np.array([1, 2]) for k in excise.COLUMNS}
    t["score"] = np.array([0.5, np.nan])
    assert excise.write_excisions_tsv(str(tmp_path / "excisions.tsv"), t) == 2
    lines = (tmp_path / "excisions.tsv").read_text().splitlines()
    assert lines[0].split("\t") == list(excise.COLUMNS) and lines[2].split("\t")[6] == "nan"


def test_block_excisions_refuse_without_gpu():
    """graal_block_excisions on a handle without a device: an error, nothing computed on the host, outputs untouched."""
    from graal_amd import build as gbuild
    from graal_amd import lib
    gbuild.build_hip()
    L = lib.load()
    h = ctypes.c_void_p()
    if L.graal_create(0, ctypes.byref(h)) == 0:
        L.graal_destroy(h)
        pytest.skip("a GPU is present: tests/test_excise_gpu.py covers the engine")
    try:
        a = np.zeros(1, np.int32); q = np.full(1, 7, np.int64); st = np.full(1, 9, np.uint8)
        rc = L.graal_block_excisions(h, 1, a.ctypes.data_as(lib._i32p), a.ctypes.data_as(lib._i32p), q.ctypes.data_as(lib._i64p),
                                     q.ctypes.data_as(lib._i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        assert rc != 0 and L.graal_last_error(h).decode() and q[0] == 7 and st[0] == 9
    finally:
        L.graal_destroy(h)
