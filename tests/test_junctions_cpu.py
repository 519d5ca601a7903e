"""Junction scores without a GPU: the numpy restatement (tests/junction_reference.py) against the oracle's dense full likelihood of each
cut layout, the table and its TSV file, and the entry points' refusal on a handle without a device (no host fallback)."""
import ctypes

import numpy as np
import pytest

import oracle.oracle as O
from graal_amd import junctions, synth
from graal_amd.lib import Engine, GraalError
from oracle.sparse_numpy import SparseScorer
from tests import junction_reference as JR


@pytest.mark.parametrize("name", ["sub3", "sub1", "circ"])
def test_reference_equals_dense_difference_of_cut_layouts(name):
    """J = dense logL(layout) - dense logL(cut layout), up to the float32 re-centring of the part that moves to a new contig.  That noise
    is measured: the sparse scorer prices the cut once with the right part re-centred and once with its old centres, and J equals the
    latter difference to 1e-7 of its terms (the scorer's own float32 powers are
    not correctly rounded)."""
    P = synth.with_dense(JR.case(name))
    dense = O.DenseOracle(P["hic_matrix"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["frag_dispatcher"],
                          P["collector_id_repeats"], P["n_frags"], P["mean_squared_frags_per_bin"], P["param_simu"], fix_trans_accu=True)
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    J, st, A = JR.reference(P)
    if name == "circ":
        assert (st[s["circ"] == 1] == JR.CIRCULAR).all()
    assert (st[(s["circ"] != 1) & (s["next"] == -1)] == JR.END).all()
    valid = np.nonzero(st == JR.VALID)[0]
    assert len(valid) >= 10
    base_d, base_s = dense.evaluate(s), sp.full(s)
    for f in valid[:: max(1, len(valid) // 12)]:
        got = J[f] / JR.Q
        cut, still = JR.cut_layout(s, int(f)), JR.cut_layout(s, int(f), recentre=False)
        exact = base_s - sp.full(still)
        assert abs(got - exact) <= 1e-7 * A[f] / JR.Q + 1e-6, (f, got, exact)   # (the scorer's float32 np.power: last-place rounding)
        noise = abs(sp.full(cut) - sp.full(still))
        want = base_d - dense.evaluate(cut)
        assert abs(got - want) <= 1.5 * noise + 1e-6 * abs(base_d), (f, got, want, noise)
    assert (J[valid] != 0).any()


def test_reference_quirk_only_moves_reversed_mixed_bins():
    """The trans-branch indexing changes J only where a reversed bin of mixed RF counts is involved; it changes nothing with RF count 9."""
    P = JR.case("circ")
    a, sa, _ = JR.reference(P)
    b, sb, _ = JR.reference(P, quirk=True)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)


def test_table_order_and_tsv(tmp_path):
    soa = {"pos": np.array([1, 0, 0, 2, 1, 0]), "id_c": np.array([4, 4, 1, 4, 1, 7]), "next": np.array([3, 0, 4, -1, -1, -1]),
           "circ": np.zeros(6, int), "ori": np.array([1, -1, 1, 1, -1, 1]), "start_bp": np.array([100, 0, 0, 250, 40, 0]),
           "len_bp": np.array([150, 100, 40, 30, 60, 10])}
    score = np.array([1.5, -2.25, 3.0, np.nan, np.nan, np.nan])
    t = junctions.table_from(soa, score)
    assert list(t["contig"]) == [1, 4, 4] and list(t["position"]) == [0, 0, 1]
    assert list(t["left_frag"]) == [2, 1, 0] and list(t["right_frag"]) == [4, 0, 3]
    assert list(t["left_ori"]) == [1, -1, 1] and list(t["right_ori"]) == [-1, 1, 1]
    assert list(t["join_bp"]) == [40, 100, 250] and list(t["score"]) == [3.0, -2.25, 1.5]
    p = tmp_path / "junctions.tsv"
    assert junctions.write_junctions_tsv(str(p), t) == 3
    lines = p.read_text().splitlines()
    assert lines[0].split("\t") == list(junctions.COLUMNS)
    assert lines[2].split("\t") == ["4", "0", "1", "0", "-1", "1", "100", "-2.25"]
    soa["circ"][:] = 1
    assert len(junctions.table_from(soa, score)["score"]) == 0


def _failed_handle():
    from graal_amd import build as gbuild
    from graal_amd import lib
    gbuild.build_hip()
    L = lib.load()
    h = ctypes.c_void_p()
    if L.graal_create(0, ctypes.byref(h)) == 0:
        L.graal_destroy(h)
        pytest.skip("a GPU is present: tests/test_junctions_gpu.py covers the engine")
    return L, h


def test_junction_scores_refuse_without_gpu():
    """graal_junction_scores and Engine.junction_scores on a handle without a device: an error, nothing computed on the host."""
    from graal_amd import lib
    L, h = _failed_handle()
    try:
        q = np.full(4, 7, np.int64)
        st = np.full(4, 9, np.uint8)
        rc = L.graal_junction_scores(h, q.ctypes.data_as(lib._i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        assert rc != 0 and L.graal_last_error(h).decode()
        assert (q == 7).all() and (st == 9).all()
        e = Engine.__new__(Engine)
        e._L, e._h, e.n = L, h, 4
        with pytest.raises(GraalError, match="graal_junction_scores"):
            e.junction_scores()
        with pytest.raises(GraalError, match="graal_junction_scores"):
            junctions.junction_table(e)
        e._h = None
    finally:
        L.graal_destroy(h)
