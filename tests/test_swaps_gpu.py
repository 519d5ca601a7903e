"""graal_block_swaps on the GPU: equal to the brute-force restatement (tests/swap_reference.py) on the small problems with the mode flag
on and off, consistent with full evaluations of the swapped layouts, its refusals, determinism and freedom from side effects on a run,
graal_amd.swaps' rounds on a simulated genome with planted transpositions, scaffold() with swap rounds, and the run module's tables."""
import os
import subprocess
import sys

import numpy as np
import pytest

from graal_amd import em, scaffold, swaps, synth
from graal_amd.lib import SWAP_CIRCULAR, SWAP_VALID, GraalError
from oracle.sparse_numpy import SparseScorer
from tests import link_reference as LR
from tests import swap_reference as SR
from tests.test_scaffold_gpu import engine_for, simulated
from tests.test_swaps_cpu import swap_sets

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = LR.case(name)
    return _CASES[name]


@pytest.mark.parametrize("name", ["sub3", "sub1", "circ"])
def test_equals_reference(name):
    """q, contacts and status of the tilings up to span 4 and of the whole-contig spans equal the brute force, with the trans-branch
    indexing off and on; q is the same integer both times."""
    P = case(name)
    s = P["S_o_A_frags"]
    R = SR.restatement(P)
    pos, lc = np.asarray(s["pos"]), np.asarray(s["l_cont"])
    sets = swap_sets(s)
    got = {}
    for quirk in (False, True):
        e = engine_for(P, quirk=quirk)
        try:
            got[quirk] = [e.block_swaps_q(*x) for x in sets]
        finally:
            e.close()
    seen = set()
    n_scored = 0
    for (first, mid, last), (q, c, st), (q1, c1, st1) in zip(sets, got[False], got[True]):
        rq, rc, rst, A = R.swaps(s, first, mid, last)
        assert np.array_equal(st, rst) and np.array_equal(c, rc)
        assert np.all(np.abs(q - rq) <= 1e-9 * A + 1), np.max(np.abs(q - rq))
        assert np.array_equal(q, q1) and np.array_equal(c, c1) and np.array_equal(st, st1)
        seen |= set(st.tolist())
        v = st == SWAP_VALID
        head, tail = pos[first] == 0, pos[last] == lc[last] - 1
        seen |= {"head"} if (v & head & ~tail).any() else set()
        seen |= {"tail"} if (v & tail & ~head).any() else set()
        seen |= {"whole"} if (v & head & tail).any() else set()
        seen |= {"one"} if (v & (first == mid) & (pos[last] == pos[mid] + 1)).any() else set()
        n_scored += int((v & (q != 0) & (c > 0)).sum())
    want = {SWAP_VALID, "head", "tail", "whole", "one"} | ({SWAP_CIRCULAR} if name == "circ" else set())
    assert want <= seen and n_scored >= 5, (seen, n_scored)


def _noise(sp, s, S, first, mid, last):
    """What the float32 re-centring moves in the full likelihood and S leaves out: the pairs inside X, inside Y and inside the rest of
    the contig, and every bin's own sub-fragment pairs (tests/test_flips_gpu._noise's construction)."""
    m, sx, sy = SR._members(s, first, mid, last)
    masks = []
    for g in (m[sx], m[sy], np.concatenate([m[:sx.start], m[sy.stop:]])):
        k = np.zeros(len(s["id_c"]), bool); k[g] = True
        masks.append(k)
    own = lambda x: sp.full(x) - sp.full(x, same_bin=False)
    return sum(abs(sp.restricted(S, k) - sp.restricted(s, k)) for k in masks) + abs(own(S) - own(s))


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("circ", True)])
def test_sampled_swaps_equal_full_evaluation_difference(name, quirk):
    """S = eval_full(swapped layout, uploaded as the restatement builds it) - eval_full(layout) for ~15 swaps, within the re-centring
    noise (the flips' tolerance)."""
    P = case(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    sets = list(swaps.tilings(s, None, 4))
    first, mid, last = (np.concatenate([x[i] for x in sets]) for i in range(3))
    e = engine_for(P, quirk=quirk)
    try:
        S_ = np.concatenate([e.block_swaps(*x)[0] for x in sets])
        assert np.isfinite(S_).all()
        e.relabel_contigs()
        base = e.eval_full()
        for i in np.unique(np.linspace(0, len(first) - 1, 15).astype(int)):
            L = SR.swap_layout(s, int(first[i]), int(mid[i]), int(last[i]))
            noise = _noise(sp, s, L, int(first[i]), int(mid[i]), int(last[i]))
            e.upload_frags(L)
            e.relabel_contigs()
            want = e.eval_full() - base
            assert abs(S_[i] - want) <= 1.5 * noise + 1e-6 * max(1.0, abs(want)), (first[i], mid[i], last[i], S_[i], want, noise)
        e.upload_frags(s)
    finally:
        e.close()


def test_refusals_leave_outputs_layout_and_state_alone():
    P = case("sub3")
    s = P["S_o_A_frags"]
    lists = LR.contigs_of(s)
    big = max(lists.values(), key=len)
    other = min((m for m in lists.values() if m[0] != big[0]), key=lambda m: m[0])
    n = len(s["id_c"])
    import ctypes
    from graal_amd.lib import _i32p, _i64p
    u8 = ctypes.POINTER(ctypes.c_uint8)
    assert len(big) >= 7
    e = engine_for(P, quirk=True)
    try:
        before = e.download_frags()
        good = (np.array([big[0], big[3]], np.int32), np.array([big[0], big[4]], np.int32), np.array([big[2], big[5]], np.int32))
        want = e.block_swaps_q(*good)
        bad = {"overlaps": ([big[0], big[4], big[2]], [big[0], big[5], big[3]], [big[1], big[6], big[5]], 2),   # swap 2 = 2..5 meets 1 = 4..6
               "overlaps ": ([big[1], big[2], big[0]], [big[1], big[2], big[0]], [big[2], big[3], big[6]], 1),  # swap 1 meets swap 0
               "two contigs": ([big[0], big[2]], [big[0], big[2]], [big[1], other[0]], 1),
               "two contigs ": ([big[0]], [other[0]], [big[1]], 0),
               "mid lies before first": ([big[3]], [big[1]], [big[5]], 0),
               "last does not lie behind mid": ([big[1]], [big[3]], [big[3]], 0),
               "last does not lie behind mid ": ([big[1]], [big[3]], [big[2]], 0),
               "out of range": ([big[0], n], [big[0], n], [big[1], n], 1),
               "out of range ": ([big[0]], [-1], [big[1]], 0)}
        for why, (first, mid, last, k) in bad.items():
            first, mid, last = (np.array(x, np.int32) for x in (first, mid, last))
            q = np.full(len(first), 7, np.int64); c = np.full(len(first), 7, np.int64); st = np.full(len(first), 9, np.uint8)
            rc = e._L.graal_block_swaps(e._h, len(first), first.ctypes.data_as(_i32p), mid.ctypes.data_as(_i32p), last.ctypes.data_as(_i32p),
                                        q.ctypes.data_as(_i64p), c.ctypes.data_as(_i64p), st.ctypes.data_as(u8))
            msg = e._L.graal_last_error(e._h).decode()
            assert rc == 1 and why.strip() in msg and "swap %d" % k in msg, (why, rc, msg)
            assert (q == 7).all() and (c == 7).all() and (st == 9).all()
        with pytest.raises(GraalError, match="overlaps"):
            e.block_swaps([big[0], big[0]], [big[0], big[0]], [big[1], big[1]])
        assert all(len(x) == 0 for x in e.block_swaps_q([], [], []))
        after = e.download_frags()
        for k in LR.FIELDS:
            assert np.array_equal(after[k], before[k]), k
        for u, v in zip(want, e.block_swaps_q(*good)):          # (a refusal leaves the next call unaffected)
            assert np.array_equal(u, v)
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.block_swaps([0], [0], [1])
    finally:
        e.close()


def test_deterministic_in_any_swap_order_and_for_an_unsorted_contact_list():
    P = case("sub3")
    s = P["S_o_A_frags"]
    first, mid, last = list(swaps.tilings(s, None, 3))[2]
    perm = np.random.RandomState(4).permutation(len(first))
    e = engine_for(P, quirk=True)
    try:
        want = e.block_swaps_q(first, mid, last)
        again = e.block_swaps_q(first, mid, last)
        shuffled = e.block_swaps_q(first[perm], mid[perm], last[perm])
        cp = np.random.RandomState(3).permutation(len(P["coo_row"]))
        e.upload_contacts(np.asarray(P["coo_row"])[cp], np.asarray(P["coo_col"])[cp], np.asarray(P["coo_val"])[cp])
        unsorted = e.block_swaps_q(first, mid, last)
    finally:
        e.close()
    assert len(first) >= 10 and np.count_nonzero(want[0]) >= 10
    for u, v, w, x in zip(want, again, shuffled, unsorted):
        assert np.array_equal(u, v) and np.array_equal(u[perm], w) and np.array_equal(u, x)


def test_no_side_effect_on_a_run():
    """run_em with block_swaps() of every pair of neighbouring fragments of the current layout (its first tiling) called at the end of
    every cycle and in the middle of one, each call followed by a refused call (an overlap), gives the same accepted moves and
    likelihoods: neither the call nor a refusal touches the step state (carried total, pending correction, proposal tables) or draws
    from the generator."""
    from tests.test_sampler_gpu import make_gpu_sampler
    P = synth.with_dense(synth.make_problem(n_bins=70, nnz=1200, n_sub=1, seed=41, contig_weights=(5, 4, 3), mean_len_bp=2000.0,
                                            param=synth.make_param_simu(fact=200.0, v_inter=0.02), grid_bp=2000))
    n = P["n_frags"]
    runs = []
    for call in (False, True):
        rng = np.random.RandomState(5)
        smp = make_gpu_sampler(P, rng, reference_arithmetic="exact")
        seen, calls = [], []

        def on_step(j, i, trace, smp=smp, seen=seen, call=call, calls=calls):
            seen.append(i)
            if call and (len(seen) % n == 0 or len(seen) == n // 2):
                e = smp.engine
                sets = list(swaps.tilings(e.download_frags(), None, 2))
                if sets:
                    first, mid, last = sets[0]
                    S, c, st = e.block_swaps(first, mid, last)
                    assert len(S) == len(first) and set(st.tolist()) <= {SWAP_VALID}
                    calls.append(len(S))
                    with pytest.raises(GraalError, match="overlaps"):        # (a refusal in the middle of a run, too)
                        e.block_swaps(first[[0, 0]], mid[[0, 0]], last[[0, 0]])

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs), rng.randint(1 << 30), len(calls)))
        smp.free_gpu()
    (m0, l0, c0, r0, _), (m1, l1, c1, r1, n_calls) = runs
    assert n_calls >= 3
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1) and r0 == r1


def spurious_and_planted(e, s):
    """On the engine's own simulated list (fetched again: the draw is a function of layout, tables, parameters and seed): the largest
    score of a swap of the TRUE layout `s` -- by the windowed restatement over the tilings up to span 4, by the engine over the
    complete tilings up to 8 -- and the gains of the planted swaps by the restatement."""
    par = synth.make_param_simu(fact=1500.0, v_inter=0.5)
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(4, 3, 2, 1), param=par)   # (simulated()'s genome)
    P["coo_row"], P["coo_col"], P["coo_val"] = e.simulate_contacts(2024)
    P["param_simu"] = par
    W = SR.window(P)
    spurious = max(W.swaps(s, *x)[0].max() / LR.Q for x in swaps.tilings(s, None, 4))
    e.upload_frags(s)
    spurious_gpu = max(np.nanmax(e.block_swaps(*x)[0]) for x in swaps.tilings(s, None, 8))
    bad, first, mid, last = SR.planted(s)
    return spurious, spurious_gpu, W.swaps(bad, first, mid, last)[0] / LR.Q


def test_swap_rounds_restore_planted_transpositions():
    """The scaffold tests' genome with the seven transpositions of tests/swap_reference.PLANTS (runs of 1 to 30 fragments):
    swap_rounds(min_score=20) restores every chromosome's order, and every kept round raises logL.  min_score must sit between two
    figures on the list this test scores, and the test asserts that first, on the engine's own list (seed 2024), and prints them.  On
    contacts drawn by numpy (seed 5; tests/test_swaps_cpu.py) the largest of the 27,440 swaps of the true layout up to 8 fragments
    scores 2.09 and the seven planted swaps gain 98.8 to 3,189.5."""
    e, s = simulated()
    try:
        spurious, spurious_gpu, gains = spurious_and_planted(e, s)
        print("largest spurious swap %.2f (span <= 4, restatement) %.2f (span <= 8, engine), planted gains %s"
              % (spurious, spurious_gpu, np.round(gains, 1).tolist()))
        assert spurious < 20.0 < gains.min() and spurious_gpu < 20.0, (spurious, spurious_gpu, gains)
        bad = SR.planted(s)[0]
        with pytest.raises(AssertionError):
            SR.assert_true_chromosomes(bad, s)
        e.upload_frags(bad)
        rec = swaps.swap_rounds(e, max_frags=8, junction_below=0.0, max_units=3, min_score=20.0)
        got = e.download_frags()
    finally:
        e.close()
    kept = [r["logL"] for r in rec if r["kept"]]
    assert len(kept) >= 2 and all(b > a for a, b in zip(kept, kept[1:])), rec
    SR.assert_true_chromosomes(got, s)


def test_scaffold_with_swaps_repairs_a_transposed_piece():
    """scaffold() alone leaves a run of three fragments that sits four places too early where it is; with swap_max_frags set, the swap
    rounds behind it move it back.  The default leaves scaffold() as it was: no swap rows."""
    e, s = simulated()
    try:
        chroms = list(LR.contig_lists(s).values())
        c0 = chroms[0]
        wrong = c0[:200] + c0[204:207] + c0[200:204] + c0[207:]
        start = LR.layout(s["len_bp"], [wrong] + chroms[1:])
        e.upload_frags(start)
        plain = scaffold.scaffold(e, rounds=5)
        got_plain = e.download_frags()
        e.upload_frags(start)
        rec = scaffold.scaffold(e, rounds=5, swap_max_frags=8, swap_min_score=20.0)
        got = e.download_frags()
    finally:
        e.close()
    assert len(rec) > len(plain) and rec[-1]["kept"] == 1 and rec[-1]["logL"] > plain[-1]["logL"]
    with pytest.raises(AssertionError):
        SR.assert_true_chromosomes(got_plain, s)
    SR.assert_true_chromosomes(got, s)


def test_run_swap_and_swaps_write_their_tables(tmp_path):
    """--swap writes its rounds, --swaps the score table of the tilings of the final layout; read back, the table equals
    Engine.block_swaps of that layout, rebuilt here by replaying the run's list_mutations.txt and running the same swap rounds."""
    from graal_amd import pyramid as pyr
    from graal_amd.sampler import sampler
    P = synth.make_problem(n_bins=300, nnz=30000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    par = synth.make_param_simu(fact=300.0, v_inter=0.02)
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    synth.write_dataset(P, data)
    cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
           "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--swap", "--swaps", "--swap-max-frags", "3",
           "--swap-min-score", "1.0", "--no-fit", "--param", *[repr(float(x)) for x in par]]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = open(os.path.join(out, "swap.tsv")).read().splitlines()
    assert lines[0].split("\t") == list(swaps.ROUND_COLUMNS) and lines[1].split("\t")[0] == "0"
    rounds = [l.split("\t") for l in lines[1:]]
    lines = open(os.path.join(out, "swaps.tsv")).read().splitlines()
    assert lines[0].split("\t") == list(swaps.COLUMNS)
    rows = [l.split("\t") for l in lines[1:]]
    ix = {c: i for i, c in enumerate(swaps.COLUMNS)}
    assert len(rows) > 0 and all(2 <= int(x[ix["frags_x"]]) + int(x[ix["frags_y"]]) <= 3 for x in rows)
    table = {(int(x[0]), int(x[1]), int(x[2])): (float(x[ix["score"]]), int(x[ix["contacts"]]), int(x[ix["status"]])) for x in rows}
    assert len(table) == len(rows)
    inp = pyr.simulation_inputs(pyr.Pyramid(os.path.join(data, "pyramids", "pyramid_1_thresh_auto"), 1), 0)
    smp = sampler(True, inp["S_o_A_frags"], inp["collector_id_repeats"], inp["frag_dispatcher"], inp["id_frag_duplicated"],
                  inp["id_frags_blacklisted"], inp["n_frags"], inp["n_new_frags"], inp["init_n_sub_frags"], inp["n_new_sub_frags"],
                  None, inp["hic_matrix_sub_sampled"], inp["np_sub_frags_len_bp"], inp["np_sub_frags_id"], inp["np_sub_frags_accu"],
                  inp["mean_squared_frags_per_bin"], inp["norm_vect_accu"], inp["S_o_A_sub_frags"], inp["hic_matrix"],
                  inp["mean_value_trans"], 1, False, None, rng=np.random.RandomState(0), reference_arithmetic="exact")
    try:
        smp.set_param_simu(np.asarray(par, dtype=np.float32))
        smp.modify_gl_cuda_buffer(0, 0)
        smp.explode_genome(0)
        em.replay(smp, em.load_mutations(os.path.join(out, "list_mutations.txt")))
        rec = swaps.swap_rounds(smp, max_frags=3, min_score=1.0)
        assert [(str(x["round"]), str(x["swaps"]), str(x["kept"])) for x in rec] == [(x[0], x[1], x[4]) for x in rounds]
        soa = smp.engine.download_frags()
        want = {}
        for first, mid, last in swaps.tilings(soa, None, 3):
            S, c, st = smp.engine.block_swaps(first, mid, last)
            want.update({(int(f), int(m), int(l)): (float(a), int(b), int(d)) for f, m, l, a, b, d in zip(first, mid, last, S, c, st)})
    finally:
        smp.free_gpu()
    assert set(want) == set(table)
    for k, (a, b, d) in want.items():
        ta, tb, td = table[k]
        assert (a == ta or (np.isnan(a) and np.isnan(ta))) and b == tb and d == td, (k, want[k], table[k])
