"""graal_end_links on the GPU: equal to the numpy restatement (tests/link_reference.py), consistent with full evaluations of the joined
layouts and with the translocation candidates' deltas, deterministic, right on a simulated genome cut into shuffled pieces, and free
of side effects on a run."""
import ctypes
import mmap
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from graal_amd import em, links, synth
from graal_amd.lib import Engine, GraalError, LINK_VALID, _i32p, _i64p
from oracle.sparse_numpy import SparseScorer
from tests import link_reference as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def engine_for(P, state=None, quirk=False):
    e = Engine(0)
    e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                      P["mean_squared_frags_per_bin"])
    e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
    e.set_params(P["param_simu"])
    e.upload_frags(P["S_o_A_frags"] if state is None else state)
    if quirk:
        e.set_mode(ref_trans_accu=True)
    return e


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = LR.case(name)
    return _CASES[name]


@pytest.mark.parametrize("name,quirk,min_frags", [("sub3", False, 1), ("sub3", True, 1), ("sub3", True, 3), ("sub1", False, 1),
                                                  ("sub1", False, 4), ("circ", False, 1), ("circ", True, 2)])
def test_equals_reference(name, quirk, min_frags):
    P = case(name)
    e = engine_for(P, quirk=quirk)
    try:
        a, b, q, c, st = e.end_links_q(min_frags)
    finally:
        e.close()
    ra, rb, rq, rc, rst, A = LR.restatement(P, quirk=quirk).links(P["S_o_A_frags"], min_frags)
    assert len(ra) >= 10
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    assert np.array_equal(st, rst) and np.array_equal(c, rc)
    assert np.all(np.abs(q - rq) <= 1e-9 * A + 1), np.max(np.abs(q - rq))


def _recentring_noise(sp, s, J, ends):
    """What the float32 re-centring moves in the full likelihood and L leaves out: the pairs of different bins inside each contig, and
    every bin's own sub-fragment pairs (a reversed bin walks its sub-fragments the other way)."""
    idc = np.asarray(s["id_c"])
    own = lambda x: sp.full(x) - sp.full(x, same_bin=False)
    return (sum(abs(sp.restricted(J, idc == idc[int(e) >> 1]) - sp.restricted(s, idc == idc[int(e) >> 1])) for e in ends)
            + abs(own(J) - own(s)))


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("circ", False), ("circ", True)])
def test_sampled_links_equal_full_evaluation_difference(name, quirk):
    """L = eval_full(joined layout) - eval_full(layout) for ~20 links, within the float32 re-centring noise of the pairs inside the two
    contigs (measured with the sparse scorer: their own pairs, and every bin's own pairs, priced in both layouts).  With the indexing
    mode on the full evaluation prices every trans pair by its lower-id bin's orientation: the mirrored mixed bins against third
    contigs are in it."""
    P = case(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    e = engine_for(P, quirk=quirk)
    try:
        a, b, L, _, st = e.end_links()
        assert (st == LINK_VALID).all()
        e.relabel_contigs()
        base = e.eval_full()
        for i in np.unique(np.linspace(0, len(a) - 1, 20).astype(int)):
            J = LR.join_layout(s, int(a[i]), int(b[i]))
            noise = _recentring_noise(sp, s, J, (a[i], b[i]))
            e.upload_frags(J)
            e.relabel_contigs()
            want = e.eval_full() - base
            assert abs(L[i] - want) <= 1.5 * noise + 1e-6 * max(1.0, abs(want)), (a[i], b[i], L[i], want, noise)
        e.upload_frags(s)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["sub3", "sub1"])
def test_translocation_candidates_equal_links(name):
    """Ops 9-12 split contig(fA) and contig(fB) at fA / fB and paste them; with fA and fB at ends of contigs of >= 2 fragments and the
    splits chosen so that they cut nothing off, the pasted layout is the canonical join (m_paste reverses A iff fA is its head, B iff fB
    is its tail).  In reference arithmetic (GRAAL_MODE_STRICT) a candidate re-prices every pixel of contig(fA) u contig(fB) from the new
    layout's float32 coordinates, as a full evaluation does: its delta is L within the same re-centring noise as eval_full's
    difference.  With the indexing mode off: the candidate's pixel set is contig(fA) u contig(fB) (as sub_compute_likelihood's), so
    under GRAAL_MODE_REF_TRANS_ACCU it would leave out the reversed mixed bins' trans pairs against third contigs that L holds."""
    P = case(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    e = engine_for(P)
    try:
        a, b, L, _, st = e.end_links()
        e.set_mode(strict=True)
        max_id = e.relabel_contigs()
        lc, pos = s["l_cont"], s["pos"]
        checked = 0
        for i in range(len(a)):
            fa, fb = int(a[i]) >> 1, int(b[i]) >> 1
            if lc[fa] < 2 or lc[fb] < 2:
                continue
            op = 9 + 2 * (1 if pos[fa] == 0 else 0) + (1 if pos[fb] == 0 else 0)
            d = e.eval_candidates(fa, [fb], max_id)[0, op]
            noise = _recentring_noise(sp, s, LR.join_layout(s, int(a[i]), int(b[i])), (a[i], b[i]))
            assert abs(L[i] - d) <= 1.5 * noise + 1e-6 * max(1.0, abs(d)), (a[i], b[i], op, L[i], d, noise)
            checked += 1
            if checked == 20:
                break
        assert checked >= 10
    finally:
        e.close()


def test_deterministic_and_cap():
    P = case("sub3")
    e = engine_for(P, quirk=True)
    try:
        x = e.end_links_q()
        y = e.end_links_q()
        for u, v in zip(x, y):
            assert np.array_equal(u, v)
        m = len(x[0])
        a = np.zeros(m, np.int32)
        q = np.zeros(m, np.int64)
        st = np.zeros(m, np.uint8)
        rc = e._L.graal_end_links_fetch(e._h, a.ctypes.data_as(_i32p), a.ctypes.data_as(_i32p), q.ctypes.data_as(_i64p),
                                        q.ctypes.data_as(_i64p), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), m - 1)
        assert rc == 1 and "cap" in e._L.graal_last_error(e._h).decode()
        with pytest.raises(GraalError, match="min_frags"):
            e.end_links(0)
    finally:
        e.close()


@pytest.mark.parametrize("seed", [2024, 7, 99])
def test_simulated_genome_best_links_are_the_true_adjacencies(seed):
    """1,000 bins in 4 chromosomes, contacts simulated from the true layout, each chromosome cut into pieces of 80 bins (about 53 kb,
    nearly 4x the 14 kb window), the pieces shuffled and about half of them reversed: every piece end with a true neighbour has that neighbour's
    end as its best link, and the mutual best links are exactly the true adjacencies."""
    par = synth.make_param_simu(fact=1500.0, v_inter=0.5)
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(4, 3, 2, 1), param=par)
    s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
    rng = np.random.RandomState(seed)
    pieces = []
    for c, frags in LR.contig_lists(s).items():
        pieces += [frags[i:i + 80] for i in range(0, len(frags), 80)]
    true = set()
    flip = rng.rand(len(pieces)) < 0.5
    def end_of(p, tail):      # the end of piece p that was its original head (tail=False) or tail, in the shuffled layout
        f = pieces[p][-1][0] if tail else pieces[p][0][0]
        return 2 * f + (int(tail) if not flip[p] else 1 - int(tail))
    for p in range(len(pieces) - 1):
        if s["id_c"][pieces[p][0][0]] == s["id_c"][pieces[p + 1][0][0]]:
            true.add(tuple(sorted((end_of(p, True), end_of(p + 1, False)))))
    shuffled = [[(f, -o) for f, o in reversed(pieces[p])] if flip[p] else pieces[p] for p in rng.permutation(len(pieces))]
    cut = LR.layout(s["len_bp"], shuffled)
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.set_params(par)
        e.upload_frags(s)
        r, c, v = e.simulate_contacts(seed)
        e.upload_contacts(r, c, v)
        e.upload_frags(cut)
        t = links.link_table(e)
    finally:
        e.close()
    assert len(true) == len(pieces) - 4 and len(t["score"]) > len(true)
    best = links.best_links(t, 1)
    got = dict(zip((2 * best["frag"] + best["side"]).tolist(), (2 * best["partner_frag"] + best["partner_side"]).tolist()))
    for x, y in true:
        assert got[x] == y and got[y] == x, (x, y, got.get(x), got.get(y))
    m = links.mutual_best(t)
    found = set(zip((2 * m["frag_a"] + m["side_a"]).tolist(), (2 * m["frag_b"] + m["side_b"]).tolist()))
    assert found == true


def _sampler(P, rng):
    from tests.test_sampler_gpu import make_gpu_sampler
    return make_gpu_sampler(P, rng, reference_arithmetic="exact")


def test_no_side_effect_on_a_run():
    """run_em with end_links() called at the end of every cycle and in the middle of one gives the same accepted moves and likelihoods."""
    P = synth.with_dense(synth.make_problem(n_bins=70, nnz=1200, n_sub=1, seed=41, contig_weights=(5, 4, 3), mean_len_bp=2000.0,
                                            param=synth.make_param_simu(fact=200.0, v_inter=0.02), grid_bp=2000))
    n = P["n_frags"]
    runs = []
    for call in (False, True):
        rng = np.random.RandomState(5)
        smp = _sampler(P, rng)
        seen = []

        def on_step(j, i, trace, smp=smp, seen=seen, call=call):
            seen.append(i)
            if call and (len(seen) % n == 0 or len(seen) == n // 2):
                smp.engine.end_links()

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs)))
        smp.free_gpu()
    (m0, l0, c0), (m1, l1, c1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1)


def test_repeats_and_ranks_refused():
    P = case("sub1")
    e = engine_for(P)
    try:
        seg = mmap.mmap(-1, max(e.exchange_bytes(2), mmap.PAGESIZE))   # (rank 0 of two: a world of one has no exchange)
        e.attach_exchange(seg, 0, 2, 0)
        with pytest.raises(GraalError, match="one rank"):
            e.end_links()
        e.detach_exchange()
        e.end_links()
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.end_links()
    finally:
        e.close()


def test_run_writes_links_tsv():
    P = synth.make_problem(n_bins=300, nnz=3000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    with tempfile.TemporaryDirectory() as d:
        data, out = os.path.join(d, "data"), os.path.join(d, "out")
        synth.write_dataset(P, data)
        cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
               "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--links", "--links-min-frags", "2",
               "--no-fit", "--param", *[str(float(x)) for x in synth.make_param_simu(fact=300.0, v_inter=0.02)]]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(os.path.join(out, "links.tsv")).read().splitlines()
        assert lines[0].split("\t") == list(links.COLUMNS)
        rows = [l.split("\t") for l in lines[1:]]
        assert len(rows) > 0
        ea = np.array([2 * int(x[1]) + int(x[2]) for x in rows]); eb = np.array([2 * int(x[4]) + int(x[5]) for x in rows])
        assert np.all(ea < eb) and np.all(np.diff(ea * 10**6 + eb) > 0)
        assert all(x[0] != x[3] and int(x[6]) > 0 and x[-1] != "nan" for x in rows)
