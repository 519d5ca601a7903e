"""The layout maps' numpy restatement (tests/map_reference.py) and the binning rule (graal_amd/csrc/map_shape.h) without a GPU: the order is
the sampler's, the observed image is image.matrix_image's, the host build of the rule agrees, the expected image conserves the sum of
lambda, and every case of tests/test_maps_gpu.py reaches what it is named for."""
import ctypes
import types

import numpy as np
import pytest

from graal_amd import image
from tests import map_reference as MR
from tests import util

CASES = ("sub3", "sub1", "circ", "wide")
_i32p = ctypes.POINTER(ctypes.c_int32)


def sampler_order(P):
    """full_order_high as sampler.display_current_matrix's own loop builds it for the case's state (the method, run on a stand-in
    object that holds what the loop reads)."""
    from graal_amd.sampler import sampler
    s = P["S_o_A_frags"]
    frags = types.SimpleNamespace(copy_from_gpu=lambda: None, **{k: np.asarray(s[k]) for k in ("id_c", "pos", "ori", "activ", "id_d")})
    me = types.SimpleNamespace(gpu_vect_frags=frags, np_sub_frags_id=np.asarray(P["np_sub_frags_id"]).reshape(-1, 4))
    return np.array(sampler.display_current_matrix(me)[2], dtype=np.int64)


@pytest.mark.parametrize("name", CASES)
def test_order_is_the_samplers(name):
    P = MR.case(name)
    order = MR.order_of(P["np_sub_frags_id"], P["S_o_A_frags"])
    assert np.array_equal(order, sampler_order(P))
    assert len(order) == P["init_n_sub_frags"] and len(np.unique(order)) == len(order)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("max_px", [4096, 50, 7])
def test_observed_is_matrix_image(name, max_px):
    P = MR.case(name)
    R = MR.reference(name, max_px)
    coo = (P["coo_row"], P["coo_col"], P["coo_val"])
    want = image.matrix_image(coo, R["order"], max_px)
    assert (R["bin"] == 1) == (max_px == 4096) and want.shape == (R["m"], R["m"])
    assert np.array_equal(R["observed"], want)
    assert want.sum() == 2.0 * np.asarray(P["coo_val"], dtype=np.float64).sum()


@pytest.mark.parametrize("S", [1, 7, 120, 144, 720])
@pytest.mark.parametrize("max_px", [1, 7, 50, 100, 4096])
def test_host_build_of_the_binning_rule(S, max_px):
    L = util.hostcheck()
    L.hc_map_shape.argtypes = [ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int, _i32p]
    L.hc_map_shape.restype = None
    ranks = np.array([0, S // 2, S - 1], dtype=np.int32)
    out = np.zeros(5, dtype=np.int32)
    L.hc_map_shape(S, max_px, ranks.ctypes.data_as(_i32p), 3, out.ctypes.data_as(_i32p))
    b, m = MR.shape(S, max_px)
    assert (int(out[0]), int(out[1])) == (b, m)
    assert list(out[2:]) == [int(r) // b for r in ranks]
    # image.matrix_image's own shape for S ranked sub-fragments
    assert image.matrix_image((np.zeros(0, int), np.zeros(0, int), np.zeros(0)), np.arange(S), max_px).shape == (m, m)
    assert m <= max_px and (m - 1) * b < S <= m * b


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("max_px", [4096, 50, 7])
def test_expected_conserves_the_sum_of_lambda(name, max_px):
    R = MR.reference(name, max_px)
    E = R["expected"]
    upper = np.triu(E, 1).sum() + 0.5 * np.trace(E)     # (a diagonal pixel holds its pairs twice)
    assert upper == pytest.approx(R["lambda_sum"], rel=1e-12)
    assert np.array_equal(E, E.T) and np.array_equal(R["terms"], R["terms"].T)
    S = len(R["order"])
    assert R["terms"].sum() == S * (S - 1)


@pytest.mark.parametrize("name", CASES)
def test_chunked_brute_force_equals_the_one_that_holds_every_pair(name):
    """map_reference.expected_chunked (the mid-size GPU tests' reference) against map_reference.reference on the small cases: the term
    counts exactly, E to 1e-12 relative (the order of the float64 additions is all that differs), every max_px in one pass, blocks of rows
    that divide neither the pixels nor the contigs.  Its far parts against a direct sum over the pairs of lambdas()."""
    P = MR.case(name)
    s = P["S_o_A_frags"]
    far_slots = (1, 8)
    got = MR.expected_chunked(P, s, MR.MAX_PX[name], far_slots, rows=37)
    a, b, lam = MR.lambdas(name)
    rec = MR.SR.sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], s)
    order, slots = MR.order_and_slots(P["np_sub_frags_id"], s)
    assert np.array_equal(order, MR.order_of(P["np_sub_frags_id"], s))
    slot_of = np.zeros(len(order), dtype=np.int64)
    slot_of[order] = slots
    f32 = np.float32
    norm = ((rec[2][a] * rec[2][b]).astype(f32) / f32(P["mean_squared_frags_per_bin"])).astype(f32)
    trans = np.maximum((f32(P["param_simu"][7]) * norm).astype(f32), f32(0)).astype(np.float64)
    cis = rec[1][a] == rec[1][b]
    for max_px in MR.MAX_PX[name]:
        R, G = MR.reference(name, max_px), got[max_px]
        assert (G["bin"], G["m"]) == (R["bin"], R["m"])
        assert np.array_equal(G["terms"], R["terms"])
        assert np.all(np.abs(G["expected"] - R["expected"]) <= 1e-12 * R["expected"])
        moved = 0
        for d in far_slots:
            w = np.where(cis & (np.abs(slot_of[a] - slot_of[b]) >= d), lam - trans, 0.0)
            want = MR.expected_from_lambda(a, b, w, R["pixel_of_sub"], R["m"])[0]
            assert np.all(np.abs(G["far"][d] - want) <= 1e-12 * R["expected"]), d
            moved += int((np.abs(want) > 1e-6 * R["expected"]).sum())
        assert moved > 0


def test_cases_reach_what_they_are_named_for():
    for name in CASES:
        P = MR.case(name)
        s = P["S_o_A_frags"]
        sid = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
        facts = {"S": int(P["init_n_sub_frags"]), "contigs": len(np.unique(s["id_c"])), "reversed": int((np.asarray(s["ori"]) == -1).sum()),
                 "multi": int((sid[:, 3] > 1).sum()), "rings": int((np.asarray(s["circ"]) == 1).sum()),
                 "accu": sorted(set(np.asarray(P["np_sub_frags_accu"]).reshape(-1, 3)[sid[:, 3][:, None] > np.arange(3)[None, :]].tolist()))}
        if name == "sub3":
            assert 130 <= facts["S"] <= 144 and facts["multi"] >= 40 and facts["reversed"] >= 10 and facts["accu"] == [1, 2, 3, 4], facts
        elif name == "sub1":
            assert facts["S"] == 120 and facts["multi"] == 0, facts
        elif name == "circ":
            assert facts["rings"] >= 10 and facts["contigs"] == 2, facts
        else:
            longest_kb, d_max, beyond, inside = MR.window_facts(P)
            assert facts["contigs"] == 3 and len(sid) == 240 and facts["multi"] >= 230 and facts["reversed"] >= 40, facts
            assert longest_kb > 3.0 * d_max, (longest_kb, d_max)
            assert beyond > inside > 10000, (beyond, inside)       # pairs beyond the window exist, and skipping them matters
            assert facts["S"] > 3 * 64 * 3                          # ranks cross wave and block boundaries (64 slots a wave, 4 waves a block)
        # the binnings: 4096 is bin 1; 50 (or 100) gives bin 2-3 with pixels that straddle fragment and contig boundaries; 7 a large bin, ragged
        straddles_contigs = False
        for max_px in MR.MAX_PX[name]:
            R = MR.reference(name, max_px)
            b, m, pix = R["bin"], R["m"], R["pixel_of_sub"]
            if max_px == 4096:
                assert b == 1 and m == facts["S"]
                continue
            if max_px == 7:
                # (a ragged last pixel everywhere but in circ, whose 133 sub-fragments are 7 x 19)
                assert m == 7 and b >= 18 and (facts["S"] % b != 0 or name == "circ"), (name, b)
            else:
                assert 2 <= b <= 15, (name, b)
            frag_of = np.zeros(facts["S"], dtype=np.int64)
            for f in range(len(sid)):
                frag_of[sid[f, :sid[f, 3]]] = f
            label_of = np.asarray(s["id_c"])[frag_of]
            per_pixel_frags = [len(set(frag_of[pix == p])) for p in range(m)]
            per_pixel_contigs = [len(set(label_of[pix == p])) for p in range(m)]
            assert max(per_pixel_frags) >= 2, (name, max_px)
            straddles_contigs = straddles_contigs or max(per_pixel_contigs) >= 2
        # (sub1's contigs hold 36, 36 and 48 sub-fragments: every bin of its list divides their boundaries; the other cases straddle them)
        assert straddles_contigs or name == "sub1", name
