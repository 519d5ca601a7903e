"""Insertions without a GPU: the numpy restatement (tests/insert_reference.py) against the sparse scorer's and a dense sum's likelihood
differences of the inserted layouts, the planner's rules (checked with tests/edit_reference.py), the TSV file, and the entry points'
refusal on a handle without a device."""
import ctypes

import numpy as np
import pytest

from graal_amd import insert
from graal_amd.lib import Engine, GraalError
from oracle.sparse_numpy import SparseScorer
from tests import edit_reference as ER
from tests import insert_reference as IR
from tests import link_reference as LR
from tests.sim_reference import sub_records


def _sample(n, k):
    return np.unique(np.linspace(0, n - 1, min(n, k)).astype(int))


def _sets(s, head, f):
    """Bin masks of P, T1 and T2 in the current layout."""
    idc, pos = np.asarray(s["id_c"]), np.asarray(s["pos"])
    return (idc == idc[head], (idc == idc[f]) & (pos <= pos[f]), (idc == idc[f]) & (pos > pos[f]))


@pytest.mark.parametrize("name,max_frags", [("sub3", 4), ("sub1", 3), ("circ", 4)])
def test_reference_equals_sparse_difference_without_recentring(name, max_frags):
    """I = full(inserted) - full(current) of the sparse scorer, with the re-centring of the pairs inside P, T1 and T2 taken out (each
    set's own pairs scored in both layouts by SparseScorer.restricted), to 1e-7 of the terms.  The sparse scorer has no trans-branch
    indexing: the mode is off here."""
    P = LR.case(name)
    s = P["S_o_A_frags"]
    p, f, r, q, c, st, A = IR.restatement(P).insertions(s, max_frags)
    assert len(p) >= 20 and (st == IR.VALID).all() and (c > 0).all()
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    base = sp.full(s, same_bin=False)
    for i in _sample(len(p), 12):
        S = IR.insert_layout(s, int(p[i]), int(f[i]), int(r[i]))
        d = sp.full(S, same_bin=False) - base
        for m in _sets(s, int(p[i]), int(f[i])):
            d -= sp.restricted(S, m) - sp.restricted(s, m)
        got = q[i] / IR.Q
        assert abs(got - d) <= 1e-7 * A[i] / IR.Q + 1e-6, (p[i], f[i], r[i], got, d)


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("sub1", True), ("circ", True)])
def test_reference_equals_dense_difference(name, quirk):
    """I = the difference of a dense sum over EVERY sub-fragment pair between the inserted layout -- its pairs inside P, T1 and T2
    priced with their old centres -- and the current layout, with the trans-branch indexing on and off (the dense oracle within its
    re-centring noise: the re-centred pairs are priced with the old centres, which is the definition)."""
    P = LR.case(name)
    s = P["S_o_A_frags"]
    R = IR.restatement(P, quirk=quirk)
    p, f, r, q, c, st, A = R.insertions(s, 3)
    assert len(p) >= 10
    centre, _, _, _ = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], s)
    base = LR.dense_loglik(R, s, LR.pricer(R, s, centre))
    for i in _sample(len(p), 8):
        S = IR.insert_layout(s, int(p[i]), int(f[i]), int(r[i]))
        cS, _, _, _ = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], S)
        fixed = [(m[R.bin_of], centre) for m in _sets(s, int(p[i]), int(f[i]))]
        d = LR.dense_loglik(R, S, LR.pricer(R, S, cS, fixed)) - base
        assert abs(q[i] / IR.Q - d) <= 1e-7 * A[i] / IR.Q + 1e-6, (p[i], f[i], r[i], q[i] / IR.Q, d)


def test_reference_quirk_moves_only_mixed_bins():
    P = LR.case("sub3")
    off = IR.restatement(P).insertions(P["S_o_A_frags"], 3)
    on = IR.restatement(P, quirk=True).insertions(P["S_o_A_frags"], 3)
    for k in (0, 1, 2, 4):
        assert np.array_equal(off[k], on[k])
    assert (off[3] != on[3]).sum() >= len(off[3]) // 2
    P = LR.case("circ")
    off, on = IR.restatement(P).insertions(P["S_o_A_frags"], 3), IR.restatement(P, quirk=True).insertions(P["S_o_A_frags"], 3)
    assert np.array_equal(off[3], on[3])


def test_insert_layout_fields():
    """The inserted layout: T keeps its label, the piece sits between f and next[f] in the asked orientation, T2 shifted by len(P)."""
    lens = np.array([100, 200, 300, 400, 500, 600, 700], np.int32)
    s = LR.layout(lens, [[(0, 1), (1, 1), (2, -1), (3, 1)], [(4, 1), (5, -1)], [(6, 1)]])
    S = IR.insert_layout(s, 4, 1, 1)
    lists = LR.contig_lists(S)
    assert sorted(lists) == [0, 2]
    assert lists[0] == [(0, 1), (1, 1), (5, 1), (4, -1), (2, -1), (3, 1)]
    assert S["start_bp"][5] == 300 and S["start_bp"][4] == 900 and S["start_bp"][2] == 1400
    assert S["l_cont_bp"][0] == 2100 and S["l_cont"][3] == 6 and S["next"][1] == 5 and S["prev"][2] == 4


def _table(rows, soa):
    p, f, r, sc = (np.array(x) for x in zip(*rows))
    return insert.table_from(soa, p, f, r, np.ones(len(p), np.int64), sc.astype(np.float64))


def _soa():
    """Contigs: A = 0..5 (label 0), B = 6..9 (label 1), pieces C = 10 (2), D = 11,12 (3), E = 13 (4), F = 14,15 (5)."""
    lens = np.full(16, 1000, np.int32)
    return LR.layout(lens, [[(i, 1) for i in range(6)], [(i, 1) for i in range(6, 10)], [(10, 1)], [(11, 1), (12, 1)], [(13, 1)],
                            [(14, 1), (15, 1)]])


def test_best_and_mutual():
    soa = _soa()
    t = _table([(10, 1, 0, 5.0), (10, 2, 1, 7.0), (11, 2, 0, 9.0), (11, 7, 1, 2.0), (13, 7, 0, 3.0), (13, 7, 1, 3.0), (14, 3, 0, np.nan),
                (14, 8, 0, -1.0)], soa)
    by_piece, by_junction = insert.best_insertions(t)
    assert by_piece == {10: 1, 11: 2, 13: 4, 14: 7}
    assert by_junction == {1: 0, 2: 2, 7: 4, 8: 7}
    assert insert.mutual_insertions(t).tolist() == [2, 4, 7]
    assert list(t["piece_frags"][[0, 2]]) == [1, 2] and list(t["next"][[0, 3]]) == [2, 8]
    assert list(t["target_contig"][[0, 3]]) == [0, 1] and list(t["piece_contig"][[0, 2]]) == [2, 3]


def test_plan_rules_and_edit():
    """Mutual-best pairs above min_score; a moved piece is not a target (the higher score stays, ties to the lower (after, piece));
    the cuts and joins are one valid graal_edit_layout batch (tests/edit_reference.py accepts it) that puts every kept piece back."""
    soa = _soa()
    # D (11,12) into A after 2 (9.0); E (13) into D after 11 (4.0): D moves, so E's insertion goes; C (10) into B after 7, reversed;
    # F (14,15) into A after 4 (1.0) is below min_score 1.5
    t = _table([(11, 2, 0, 9.0), (13, 11, 0, 4.0), (10, 7, 1, 6.0), (14, 4, 1, 1.0)], soa)
    cuts, joins, rows = insert.plan_insertions(t, soa, 1.5)
    assert rows.tolist() == [0, 2] and cuts.tolist() == [2, 7]
    assert joins.tolist() == [[5, 22], [25, 6], [15, 21], [20, 16]]
    new, st = ER.edit(soa, cuts, joins)
    assert new is not None, st
    lists = LR.contig_lists(new)
    chains = sorted([f for f, _ in v] for v in lists.values())
    assert [0, 1, 2, 11, 12, 3, 4, 5] in chains and ([6, 7, 10, 8, 9] in chains or [9, 8, 10, 7, 6] in chains)
    # a tie: the lower (after, piece) stays
    t = _table([(11, 2, 0, 4.0), (13, 11, 0, 4.0)], soa)
    assert insert.plan_insertions(t, soa, 0.0)[2].tolist() == [0]
    t = _table([(13, 11, 0, 4.0), (11, 2, 0, 4.0)], soa)
    assert insert.plan_insertions(t, soa, 0.0)[2].tolist() == [1]
    # several insertions into one contig, neighbouring junctions included: a matching, no cycle
    t = _table([(10, 1, 0, 3.0), (13, 2, 1, 2.0), (14, 4, 0, 5.0)], soa)
    cuts, joins, rows = insert.plan_insertions(t, soa, 0.0)
    new, st = ER.edit(soa, cuts, joins)
    assert new is not None and len(rows) == 3, st
    chains = sorted([f for f, _ in v] for v in LR.contig_lists(new).values())
    assert [0, 1, 10, 2, 13, 3, 4, 14, 15, 5] in chains or [5, 15, 14, 4, 3, 13, 2, 10, 1, 0] in chains


def test_tsv(tmp_path):
    soa = _soa()
    t = _table([(11, 2, 0, 9.0), (10, 7, 1, np.nan)], soa)
    path = tmp_path / "insertions.tsv"
    assert insert.write_insertions_tsv(str(path), t) == 2
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == list(insert.COLUMNS)
    assert lines[1].split("\t") == ["3", "11", "2", "0", "2", "3", "0", "1", "9.0"]
    assert lines[2].split("\t")[-1] == "nan"


def _failed_handle():
    from graal_amd import build as gbuild
    from graal_amd import lib
    gbuild.build_hip()
    L = lib.load()
    h = ctypes.c_void_p()
    if L.graal_create(0, ctypes.byref(h)) == 0:
        L.graal_destroy(h)
        pytest.skip("a GPU is present: tests/test_insert_gpu.py covers the engine")
    return L, h


def test_insertions_refuse_without_gpu():
    """graal_insertions, its fetch and Engine.insertions on a handle without a device: an error, nothing computed on the host."""
    from graal_amd import lib
    L, h = _failed_handle()
    try:
        m = ctypes.c_int64(7)
        rc = L.graal_insertions(h, 1, ctypes.byref(m))
        assert rc != 0 and L.graal_last_error(h).decode() and m.value == 7
        a = np.full(4, 7, np.int32)
        q = np.full(4, 7, np.int64)
        b = np.full(4, 9, np.uint8)
        u8 = ctypes.POINTER(ctypes.c_uint8)
        rc = L.graal_insertions_fetch(h, a.ctypes.data_as(lib._i32p), a.ctypes.data_as(lib._i32p), b.ctypes.data_as(u8),
                                      q.ctypes.data_as(lib._i64p), q.ctypes.data_as(lib._i64p), b.ctypes.data_as(u8), 4)
        assert rc != 0 and (a == 7).all() and (q == 7).all() and (b == 9).all()
        e = Engine.__new__(Engine)
        e._L, e._h, e.n = L, h, 4
        with pytest.raises(GraalError, match="graal_insertions"):
            e.insertions(1)
        with pytest.raises(GraalError, match="graal_insertions"):
            insert.insertion_table(e, 1)
        e._h = None
    finally:
        L.graal_destroy(h)
