"""graal_insertions on the GPU: equal to the numpy restatement (tests/insert_reference.py), consistent with full evaluations of the
inserted layouts, deterministic and free of side effects on a run, its refusals, and graal_amd.scaffold's insertion step on a simulated
genome with small pieces cut out of its chromosomes."""
import ctypes
import mmap
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from graal_amd import em, insert, scaffold, synth
from graal_amd.lib import GraalError, INSERT_VALID, _i32p, _i64p
from oracle.sparse_numpy import SparseScorer
from tests import insert_reference as IR
from tests import link_reference as LR
from tests.test_scaffold_gpu import assert_true_chromosomes, engine_for, simulated

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_u8p = ctypes.POINTER(ctypes.c_uint8)

_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = LR.case(name)
    return _CASES[name]


@pytest.mark.parametrize("name,quirk,max_frags", [("sub3", False, 1), ("sub3", True, 4), ("sub3", False, 4), ("sub1", False, 4),
                                                  ("sub1", True, 1), ("circ", True, 4)])
def test_equals_reference(name, quirk, max_frags):
    P = case(name)
    s = P["S_o_A_frags"]
    e = engine_for(P, quirk=quirk)
    try:
        p, f, r, q, c, st = e.insertions_q(max_frags)
    finally:
        e.close()
    rp, rf, rr, rq, rc, rst, A = IR.restatement(P, quirk=quirk).insertions(s, max_frags)
    assert len(rp) >= 20
    assert np.array_equal(p, rp) and np.array_equal(f, rf) and np.array_equal(r, rr)
    assert np.array_equal(st, rst) and np.array_equal(c, rc)
    assert np.all(np.abs(q - rq) <= 1e-9 * A + 1), np.max(np.abs(q - rq))
    # coverage: both orientations, junctions at T's first fragment (T1 one fragment) and before its last (T2 one fragment)
    pos, lc = np.asarray(s["pos"]), np.asarray(s["l_cont"])
    assert set(r.tolist()) == {0, 1}
    assert (pos[f] == 0).any() and (pos[f] == lc[f] - 2).any()
    if max_frags > 1:
        assert (lc[p] > 1).any() and (lc[p] == 1).any()


def _noise(sp, s, S, head, f):
    """What the float32 re-centring moves in the full likelihood and I leaves out: the pairs inside P, T1 and T2, and every bin's own
    sub-fragment pairs (a reversed bin walks its sub-fragments the other way)."""
    idc, pos = np.asarray(s["id_c"]), np.asarray(s["pos"])
    sets = (idc == idc[head], (idc == idc[f]) & (pos <= pos[f]), (idc == idc[f]) & (pos > pos[f]))
    own = lambda x: sp.full(x) - sp.full(x, same_bin=False)
    return sum(abs(sp.restricted(S, m) - sp.restricted(s, m)) for m in sets) + abs(own(S) - own(s))


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("circ", True)])
def test_sampled_insertions_equal_full_evaluation_difference(name, quirk):
    """I = eval_full(inserted layout, uploaded as the restatement builds it) - eval_full(layout) for ~15 candidates, within the
    re-centring noise (links' tolerance)."""
    P = case(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    e = engine_for(P, quirk=quirk)
    try:
        p, f, r, I, _, st = e.insertions(3)
        assert (st == INSERT_VALID).all()
        e.relabel_contigs()
        base = e.eval_full()
        for i in np.unique(np.linspace(0, len(p) - 1, 15).astype(int)):
            S = IR.insert_layout(s, int(p[i]), int(f[i]), int(r[i]))
            noise = _noise(sp, s, S, int(p[i]), int(f[i]))
            e.upload_frags(S)
            e.relabel_contigs()
            want = e.eval_full() - base
            assert abs(I[i] - want) <= 1.5 * noise + 1e-6 * max(1.0, abs(want)), (p[i], f[i], r[i], I[i], want, noise)
        e.upload_frags(s)
    finally:
        e.close()


def test_deterministic_cap_and_refusals():
    P = case("sub3")
    e = engine_for(P, quirk=True)
    try:
        before = e.download_frags()
        x = e.insertions_q(3)
        y = e.insertions_q(3)
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
        m = len(x[0])
        a = np.zeros(m, np.int32)
        q = np.zeros(m, np.int64)
        b = np.zeros(m, np.uint8)
        rc = e._L.graal_insertions_fetch(e._h, a.ctypes.data_as(_i32p), a.ctypes.data_as(_i32p), b.ctypes.data_as(_u8p),
                                         q.ctypes.data_as(_i64p), q.ctypes.data_as(_i64p), b.ctypes.data_as(_u8p), m - 1)
        assert rc == 1 and "cap" in e._L.graal_last_error(e._h).decode()
        with pytest.raises(GraalError, match="max_piece_frags"):
            e.insertions(0)
        seg = mmap.mmap(-1, max(e.exchange_bytes(2), mmap.PAGESIZE))
        e.attach_exchange(seg, 0, 2, 0)
        with pytest.raises(GraalError, match="one rank"):
            e.insertions(1)
        e.detach_exchange()
        after = e.download_frags()
        for k in LR.FIELDS:
            assert np.array_equal(after[k], before[k]), k
        z = e.insertions_q(3)                                   # (a refusal leaves the last table's computation unaffected)
        for u, v in zip(x, z):
            assert np.array_equal(u, v)
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.insertions(1)
    finally:
        e.close()


def test_unsorted_contact_list_gives_the_same_table():
    """graal_upload_contacts takes the list in any order: a shuffled copy gives the same table, bit for bit."""
    P = case("sub3")
    e = engine_for(P, quirk=True)
    try:
        want = e.insertions_q(4)
        perm = np.random.RandomState(3).permutation(len(P["coo_row"]))
        e.upload_contacts(np.asarray(P["coo_row"])[perm], np.asarray(P["coo_col"])[perm], np.asarray(P["coo_val"])[perm])
        got = e.insertions_q(4)
        again = e.insertions_q(4)
    finally:
        e.close()
    assert len(want[0]) >= 20
    for u, v, w in zip(want, got, again):
        assert np.array_equal(u, v) and np.array_equal(u, w)


def test_no_side_effect_on_a_run():
    """run_em with insertions() called at the end of every cycle and in the middle of one, each call followed by two refused calls
    (max_piece_frags 0, a fetch with a cap too small), gives the same accepted moves and likelihoods: neither the call nor a refusal
    touches the step state (carried total, pending correction)."""
    from tests.test_sampler_gpu import make_gpu_sampler
    P = synth.with_dense(synth.make_problem(n_bins=70, nnz=1200, n_sub=1, seed=41, contig_weights=(5, 4, 3), mean_len_bp=2000.0,
                                            param=synth.make_param_simu(fact=200.0, v_inter=0.02), grid_bp=2000))
    n = P["n_frags"]
    runs = []
    for call in (False, True):
        rng = np.random.RandomState(5)
        smp = make_gpu_sampler(P, rng, reference_arithmetic="exact")
        seen = []

        def on_step(j, i, trace, smp=smp, seen=seen, call=call):
            seen.append(i)
            if call and (len(seen) % n == 0 or len(seen) == n // 2):
                e = smp.engine
                e.insertions(3)
                with pytest.raises(GraalError, match="max_piece_frags"):     # (refusals in the middle of a run, too)
                    e.insertions(0)
                a = np.zeros(1, np.int32)
                q = np.zeros(1, np.int64)
                b = np.zeros(1, np.uint8)
                rc = e._L.graal_insertions_fetch(e._h, a.ctypes.data_as(_i32p), a.ctypes.data_as(_i32p), b.ctypes.data_as(_u8p),
                                                 q.ctypes.data_as(_i64p), q.ctypes.data_as(_i64p), b.ctypes.data_as(_u8p), -1)
                assert rc == 1

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs)))
        smp.free_gpu()
    (m0, l0, c0), (m1, l1, c1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1)


def cut_pieces(s, seed):
    """The true chromosomes with 8 pieces of 1-3 fragments cut out of interior positions (>= 40 bins, about twice the window, from a
    chromosome end and from each other), each piece its own contig, about half of them reversed; each chromosome closed over its gaps."""
    rng = np.random.RandomState(seed)
    chroms = [list(v) for v in LR.contig_lists(s).values()]
    spots = {0: 3, 1: 3, 2: 2}
    pieces, closed = [], []
    for ci, frags in enumerate(chroms):
        k = spots.get(ci, 0)
        taken = set()
        if k:
            bounds = np.linspace(40, len(frags) - 40, k + 1).astype(int)
            for a, b in zip(bounds[:-1], bounds[1:]):
                w = int(rng.randint(1, 4))
                at = int(rng.randint(a + 20, b - 20 - w))
                piece = frags[at:at + w]
                if rng.rand() < 0.5:
                    piece = [(x, -o) for x, o in reversed(piece)]
                pieces.append(piece)
                taken.update(range(at, at + w))
        closed.append([fr for i, fr in enumerate(frags) if i not in taken])
    return LR.layout(s["len_bp"], closed + pieces), len(pieces)


@pytest.mark.parametrize("seed", [2024, 7, 99])
def test_insertion_scaffolding_puts_the_pieces_back(seed):
    e, s = simulated()
    try:
        cut, n_pieces = cut_pieces(s, seed)
        e.upload_frags(cut)
        rec = scaffold.scaffold(e, rounds=20, insert_max_frags=3)
        got = e.download_frags()
        e.upload_frags(cut)
        plain = scaffold.scaffold(e, rounds=20)
        got_plain = e.download_frags()
    finally:
        e.close()
    kept = [r["logL"] for r in rec if r["kept"]]
    assert all(b >= a for a, b in zip(kept, kept[1:])), rec
    assert_true_chromosomes(got, s)
    with pytest.raises(AssertionError):
        assert_true_chromosomes(got_plain, s)
    assert len(np.unique(got_plain["id_c"])) > 4, plain


def test_run_insert_and_insertions_write_their_tables():
    """--insert writes its rounds in the scaffold record's format; --insertions (without --insert: the MCMC's final layout still holds
    small contigs) writes the table of the final layout."""
    P = synth.make_problem(n_bins=300, nnz=30000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    with tempfile.TemporaryDirectory() as d:
        data = os.path.join(d, "data")
        synth.write_dataset(P, data)
        for extra in (["--insert"], ["--insertions", "--insert-max-frags", "40"]):
            out = os.path.join(d, extra[0][2:])
            cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
                   "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, *extra,
                   "--no-fit", "--param", *[str(float(x)) for x in synth.make_param_simu(fact=300.0, v_inter=0.02)]]
            r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
        lines = open(os.path.join(d, "insert", "insert.tsv")).read().splitlines()
        assert lines[0].split("\t") == list(scaffold.COLUMNS)
        assert lines[1].split("\t")[0] == "0" and len(lines) >= 3
        lines = open(os.path.join(d, "insertions", "insertions.tsv")).read().splitlines()
        assert lines[0].split("\t") == list(insert.COLUMNS)
        rows = [l.split("\t") for l in lines[1:]]
        assert len(rows) > 0
        key = [(int(x[4]), int(x[1]), int(x[6])) for x in rows]
        assert key == sorted(key) and len(set(key)) == len(key)
        assert all(x[0] != x[3] and int(x[2]) <= 40 and int(x[7]) > 0 for x in rows)
