"""End links without a GPU: the numpy restatement (tests/link_reference.py) against the sparse scorer's and a dense sum's likelihood
differences of the joined layouts, the table helpers and their TSV file, and the entry points' refusal on a handle without a device."""
import ctypes

import numpy as np
import pytest

from graal_amd import links
from graal_amd.lib import Engine, GraalError
from oracle.sparse_numpy import SparseScorer
from tests import link_reference as LR
from tests.sim_reference import sub_records


def _sample(n, k):
    return np.unique(np.linspace(0, n - 1, min(n, k)).astype(int))


@pytest.mark.parametrize("name", ["sub3", "sub1", "circ"])
def test_reference_equals_sparse_difference_without_recentring(name):
    """L = full(joined) - full(current) of the sparse scorer, with the re-centring of the pairs inside A and inside B taken out (each
    contig's own pairs scored in both layouts by SparseScorer.restricted), to 1e-7 of the terms (the scorer's float32 powers are not
    correctly rounded).  The sparse scorer has no trans-branch indexing: the mode is off here."""
    P = LR.case(name)
    s = P["S_o_A_frags"]
    R = LR.restatement(P)
    a, b, q, c, st, A = R.links(s)
    assert len(a) >= 20 and (st == LR.VALID).all() and (c > 0).all()
    assert np.all(a < b) and np.all(np.diff(a * 10**6 + b) > 0)
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    base = sp.full(s, same_bin=False)
    idc = np.asarray(s["id_c"])
    for i in _sample(len(a), 12):
        J = LR.join_layout(s, int(a[i]), int(b[i]))
        d = sp.full(J, same_bin=False) - base
        for f in (int(a[i]) >> 1, int(b[i]) >> 1):
            inset = idc == idc[f]
            d -= sp.restricted(J, inset) - sp.restricted(s, inset)
        got = q[i] / LR.Q
        assert abs(got - d) <= 1e-7 * A[i] / LR.Q + 1e-6, (a[i], b[i], got, d)


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("circ", True)])
def test_reference_equals_dense_difference(name, quirk):
    """L = the difference of a dense sum over EVERY sub-fragment pair (contacts and expected mass) between the joined layout, its pairs
    inside A and inside B priced with their old centres, and the current layout -- with the trans-branch indexing on and off.  The dense
    sum has no notion of which pairs a join changes: the mirrored mixed bins against the third contigs are in it."""
    P = LR.case(name)
    s = P["S_o_A_frags"]
    R = LR.restatement(P, quirk=quirk)
    a, b, q, c, st, A = R.links(s)
    centre, _, _, _ = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], s)
    base = LR.dense_loglik(R, s, LR.pricer(R, s, centre))
    lab = np.asarray(s["id_c"])[R.bin_of]
    for i in _sample(len(a), 10):
        J = LR.join_layout(s, int(a[i]), int(b[i]))
        cJ, _, _, _ = sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], J)
        fixed = [(lab == lab[R.bin_of == (int(e) >> 1)][0], centre) for e in (a[i], b[i])]
        d = LR.dense_loglik(R, J, LR.pricer(R, J, cJ, fixed)) - base
        assert abs(q[i] / LR.Q - d) <= 1e-7 * A[i] / LR.Q + 1e-6, (a[i], b[i], q[i] / LR.Q, d)


def test_reference_quirk_moves_only_mixed_bins():
    """The trans-branch indexing changes L where mixed RF counts are involved (n_sub 3, RF counts 1..4), and nowhere with RF count 9."""
    P = LR.case("sub3")
    off = LR.restatement(P).links(P["S_o_A_frags"])
    on = LR.restatement(P, quirk=True).links(P["S_o_A_frags"])
    assert np.array_equal(off[0], on[0]) and np.array_equal(off[1], on[1]) and np.array_equal(off[3], on[3])
    assert (off[2] != on[2]).sum() >= len(off[2]) // 2
    P = LR.case("circ")
    off, on = LR.restatement(P).links(P["S_o_A_frags"]), LR.restatement(P, quirk=True).links(P["S_o_A_frags"])
    assert np.array_equal(off[2], on[2])


def test_reference_min_frags_and_rings():
    """min_frags drops every link of a shorter contig; a ring has no ends."""
    P = LR.case("circ")
    s = P["S_o_A_frags"]
    ring = set(np.nonzero(np.asarray(s["circ"]) == 1)[0].tolist())
    R = LR.restatement(P)
    a, b, *_ = R.links(s)
    assert not ({int(e) >> 1 for e in np.concatenate([a, b])} & ring)
    a4, b4, *_ = R.links(s, min_frags=4)
    lc = np.asarray(s["l_cont"])
    keep = (lc[a >> 1] >= 4) & (lc[b >> 1] >= 4)
    assert 0 < len(a4) < len(a) and np.array_equal(a4, a[keep]) and np.array_equal(b4, b[keep])


def _table():
    soa = {"id_c": np.array([3, 3, 5, 8, 8, 9])}
    #          ends:  0/1 frag0  2/3 frag1  4/5 frag2  6/7 frag3  8/9 frag4  10/11 frag5
    ea = np.array([1, 1, 1, 3, 4, 5, 6])
    eb = np.array([4, 6, 10, 8, 10, 9, 11])
    score = np.array([5.0, 2.0, np.nan, 7.0, 1.0, -3.0, 0.5])
    cnt = np.array([10, 4, 2, 12, 3, 1, 2])
    return links.table_from(soa, ea, eb, cnt, score)


def test_table_best_and_mutual():
    t = _table()
    assert list(t["contig_a"]) == [3, 3, 3, 3, 5, 5, 8] and list(t["frag_b"]) == [2, 3, 5, 4, 5, 4, 5]
    assert list(t["side_a"]) == [1, 1, 1, 1, 0, 1, 0] and list(t["side_b"]) == [0, 0, 0, 0, 0, 1, 1]
    b = links.best_links(t, 2)
    ends = 2 * b["frag"] + b["side"]
    assert list(ends) == [1, 1, 3, 4, 4, 5, 6, 6, 8, 9, 10, 11]
    assert list(b["rank"]) == [0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0]
    assert list(2 * b["partner_frag"] + b["partner_side"]) == [4, 6, 8, 1, 10, 9, 1, 11, 3, 5, 4, 6]
    assert list(b["score"][:2]) == [5.0, 2.0] and b["contig"][0] == 3 and b["partner_contig"][0] == 5
    m = links.mutual_best(t)
    # 1 <-> 4 (5.0) and 3 <-> 8 (7.0) are mutual; 6's best is 1 (taken by 4); 5 <-> 9 is mutual but negative
    assert list(2 * m["frag_a"] + m["side_a"]) == [1, 3] and list(2 * m["frag_b"] + m["side_b"]) == [4, 8]
    assert set(m) == set(links.COLUMNS)
    assert len(links.best_links(t, 0)["frag"]) == 0


def test_tsv(tmp_path):
    t = _table()
    p = tmp_path / "links.tsv"
    assert links.write_links_tsv(str(p), t) == 7
    lines = p.read_text().splitlines()
    assert lines[0].split("\t") == list(links.COLUMNS)
    assert lines[1].split("\t") == ["3", "0", "1", "5", "2", "0", "10", "5.0"]
    assert lines[3].split("\t")[-1] == "nan"


def _failed_handle():
    from graal_amd import build as gbuild
    from graal_amd import lib
    gbuild.build_hip()
    L = lib.load()
    h = ctypes.c_void_p()
    if L.graal_create(0, ctypes.byref(h)) == 0:
        L.graal_destroy(h)
        pytest.skip("a GPU is present: tests/test_links_gpu.py covers the engine")
    return L, h


def test_end_links_refuse_without_gpu():
    """graal_end_links, its fetch and Engine.end_links on a handle without a device: an error, nothing computed on the host."""
    from graal_amd import lib
    L, h = _failed_handle()
    try:
        m = ctypes.c_int64(7)
        rc = L.graal_end_links(h, 1, ctypes.byref(m))
        assert rc != 0 and L.graal_last_error(h).decode() and m.value == 7
        a = np.full(4, 7, np.int32)
        q = np.full(4, 7, np.int64)
        st = np.full(4, 9, np.uint8)
        rc = L.graal_end_links_fetch(h, a.ctypes.data_as(lib._i32p), a.ctypes.data_as(lib._i32p), q.ctypes.data_as(lib._i64p),
                                     q.ctypes.data_as(lib._i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), 4)
        assert rc != 0 and (a == 7).all() and (q == 7).all() and (st == 9).all()
        e = Engine.__new__(Engine)
        e._L, e._h, e.n = L, h, 4
        with pytest.raises(GraalError, match="graal_end_links"):
            e.end_links()
        with pytest.raises(GraalError, match="graal_end_links"):
            links.link_table(e)
        e._h = None
    finally:
        L.graal_destroy(h)
