"""graal_block_flips on the GPU: equal to the brute-force restatement (tests/flip_reference.py) on the small problems, consistent with
full evaluations of the flipped layouts, its refusals, determinism and freedom from side effects on a run, and graal_amd.flips' rounds
on a simulated genome with planted inversions."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from graal_amd import em, flips, scaffold, synth
from graal_amd.lib import FLIP_CIRCULAR, FLIP_VALID, FLIP_WHOLE, GraalError
from oracle.sparse_numpy import SparseScorer
from tests import flip_reference as FR
from tests import link_reference as LR
from tests.flip_reference import assert_true_chromosomes_and_orientations, planted
from tests.test_scaffold_gpu import engine_for, simulated

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CASES = {}
CASES = [(n, q) for n in ("sub3", "sub1", "circ") for q in (False, True)]


def case(name):
    if name not in _CASES:
        _CASES[name] = LR.case(name)
    return _CASES[name]


def block_sets(s):
    """The tilings up to 4 fragments, then one call with every linear contig of >= 2 fragments whole and, in a ring, two blocks."""
    sets = list(flips.tilings(s, None, 4))
    circ = np.asarray(s["circ"])
    first, last = [], []
    for m in LR.contigs_of(s).values():
        if circ[m[0]] == 1:
            first += [m[0], m[3]]; last += [m[1], m[3]]
        elif len(m) >= 2:
            first.append(m[0]); last.append(m[-1])
    sets.append((np.array(first, np.int32), np.array(last, np.int32)))
    return sets


@pytest.mark.parametrize("name,quirk", CASES)
def test_equals_reference(name, quirk):
    P = case(name)
    s = P["S_o_A_frags"]
    R = FR.restatement(P, quirk=quirk)
    pos, lc = np.asarray(s["pos"]), np.asarray(s["l_cont"])
    seen = set()
    e = engine_for(P, quirk=quirk)
    try:
        got = [e.block_flips_q(first, last) for first, last in block_sets(s)]
    finally:
        e.close()
    for (first, last), (q, c, st) in zip(block_sets(s), got):
        rq, rc, rst, A = R.flips(s, first, last)
        assert np.array_equal(st, rst) and np.array_equal(c, rc)
        assert np.all(np.abs(q - rq) <= 1e-9 * A + 1), np.max(np.abs(q - rq))
        seen |= set(st.tolist())
        v = st == FLIP_VALID
        seen |= {"head"} if (v & (pos[first] == 0)).any() else set()
        seen |= {"tail"} if (v & (pos[last] == lc[last] - 1)).any() else set()
        seen |= {"one"} if (v & (first == last)).any() else set()
        seen |= {"scored"} if (v & (q != 0) & (c > 0)).sum() >= 5 else set()
    want = {FLIP_VALID, FLIP_WHOLE, "head", "tail", "one", "scored"} | ({FLIP_CIRCULAR} if name == "circ" else set())
    assert want <= seen, seen


def _noise(sp, s, S, first, last):
    """What the float32 re-centring moves in the full likelihood and F leaves out: the pairs inside the block and inside the rest of its
    contig, and every bin's own sub-fragment pairs (a reversed bin walks its sub-fragments the other way)."""
    m, sl = FR._members(s, first, last)
    in_b = np.zeros(len(s["id_c"]), bool); in_b[m[sl]] = True
    in_r = (np.asarray(s["id_c"]) == np.asarray(s["id_c"])[first]) & ~in_b
    own = lambda x: sp.full(x) - sp.full(x, same_bin=False)
    return sum(abs(sp.restricted(S, k) - sp.restricted(s, k)) for k in (in_b, in_r)) + abs(own(S) - own(s))


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("circ", True)])
def test_sampled_flips_equal_full_evaluation_difference(name, quirk):
    """F = eval_full(flipped layout, uploaded as the restatement builds it) - eval_full(layout) for ~15 blocks, within the re-centring
    noise (insertions' tolerance)."""
    P = case(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    sets = list(flips.tilings(s, None, 4))
    first, last = np.concatenate([a for a, _ in sets]), np.concatenate([b for _, b in sets])
    e = engine_for(P, quirk=quirk)
    try:
        F = np.concatenate([e.block_flips(a, b)[0] for a, b in sets])
        assert np.isfinite(F).all()
        e.relabel_contigs()
        base = e.eval_full()
        for i in np.unique(np.linspace(0, len(first) - 1, 15).astype(int)):
            S = FR.flip_layout(s, int(first[i]), int(last[i]))
            noise = _noise(sp, s, S, int(first[i]), int(last[i]))
            e.upload_frags(S)
            e.relabel_contigs()
            want = e.eval_full() - base
            assert abs(F[i] - want) <= 1.5 * noise + 1e-6 * max(1.0, abs(want)), (first[i], last[i], F[i], want, noise)
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
    e = engine_for(P, quirk=True)
    try:
        before = e.download_frags()
        good = (np.array([big[0], big[3]], np.int32), np.array([big[1], big[5]], np.int32))
        want = e.block_flips_q(*good)
        bad = {"overlaps": ([big[0], big[4], big[2]], [big[1], big[6], big[5]], 2),      # block 2 = positions 2..5 meets block 1 = 4..6
               "overlaps ": ([big[1], big[2], big[0]], [big[2], big[3], big[6]], 1),   # block 1 meets block 0 before the long block 2 comes
               "two contigs": ([big[0], big[2]], [big[1], other[0]], 1),
               "before first": ([big[3]], [big[1]], 0),
               "out of range": ([big[0], n], [big[1], n], 1),
               "out of range ": ([-1], [big[1]], 0)}
        for why, (first, last, k) in bad.items():
            first, last = np.array(first, np.int32), np.array(last, np.int32)
            q = np.full(len(first), 7, np.int64); c = np.full(len(first), 7, np.int64); st = np.full(len(first), 9, np.uint8)
            rc = e._L.graal_block_flips(e._h, len(first), first.ctypes.data_as(_i32p), last.ctypes.data_as(_i32p), q.ctypes.data_as(_i64p),
                                        c.ctypes.data_as(_i64p), st.ctypes.data_as(u8))
            msg = e._L.graal_last_error(e._h).decode()
            assert rc == 1 and why.strip() in msg and "block %d" % k in msg, (why, rc, msg)
            assert (q == 7).all() and (c == 7).all() and (st == 9).all()
        with pytest.raises(GraalError, match="overlaps"):
            e.block_flips([big[0], big[0]], [big[0], big[0]])
        assert all(len(x) == 0 for x in e.block_flips_q([], []))
        after = e.download_frags()
        for k in LR.FIELDS:
            assert np.array_equal(after[k], before[k]), k
        for u, v in zip(want, e.block_flips_q(*good)):          # (a refusal leaves the next call unaffected)
            assert np.array_equal(u, v)
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.block_flips([0], [0])
    finally:
        e.close()


def test_deterministic_in_any_block_order_and_for_an_unsorted_contact_list():
    P = case("sub3")
    s = P["S_o_A_frags"]
    first, last = list(flips.tilings(s, None, 3))[3]
    perm = np.random.RandomState(4).permutation(len(first))
    e = engine_for(P, quirk=True)
    try:
        want = e.block_flips_q(first, last)
        again = e.block_flips_q(first, last)
        shuffled = e.block_flips_q(first[perm], last[perm])
        cp = np.random.RandomState(3).permutation(len(P["coo_row"]))
        e.upload_contacts(np.asarray(P["coo_row"])[cp], np.asarray(P["coo_col"])[cp], np.asarray(P["coo_val"])[cp])
        unsorted = e.block_flips_q(first, last)
    finally:
        e.close()
    assert len(first) >= 10 and np.count_nonzero(want[0]) >= 10
    for u, v, w, x in zip(want, again, shuffled, unsorted):
        assert np.array_equal(u, v) and np.array_equal(u[perm], w) and np.array_equal(u, x)


def test_no_side_effect_on_a_run():
    """run_em with block_flips() of every one-fragment block (valid in any layout) called at the end of every cycle and in the middle
    of one, each call followed by a refused call (an overlap), gives the same accepted moves and likelihoods: neither the call nor a
    refusal touches the step state (carried total, pending correction, proposal tables) or draws from the generator."""
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
                F, c, st = e.block_flips(np.arange(n), np.arange(n))
                assert len(F) == n and set(st.tolist()) <= {FLIP_VALID, FLIP_WHOLE, FLIP_CIRCULAR}
                with pytest.raises(GraalError, match="overlaps"):        # (a refusal in the middle of a run, too)
                    e.block_flips([0, 0], [0, 0])

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs), rng.randint(1 << 30)))
        smp.free_gpu()
    (m0, l0, c0, r0), (m1, l1, c1, r1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1) and r0 == r1


def spurious_and_planted(e, s):
    """On the engine's own simulated list (fetched again: the draw is a function of layout, tables, parameters and seed), with the
    windowed restatement: the largest score of a run of 2-8 fragments of the TRUE layout `s`, and the gains of the planted blocks."""
    par = synth.make_param_simu(fact=1500.0, v_inter=0.5)
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(4, 3, 2, 1), param=par)   # (simulated()'s genome)
    P["coo_row"], P["coo_col"], P["coo_val"] = e.simulate_contacts(2024)
    P["param_simu"] = par
    W = FR.window(P)
    spurious = -np.inf
    for first, last in flips.tilings(s, None, 8):
        q = W.flips(s, first, last)[0][first != last]
        spurious = max(spurious, q.max() / LR.Q) if len(q) else spurious
    bad, first, last = planted(s)
    return spurious, W.flips(bad, last, first)[0] / LR.Q             # (in the planted layout a block starts at its old last fragment)


def test_flip_rounds_restore_planted_inversions():
    """The scaffold tests' genome with the seven inversions of tests/flip_reference.PLANTS (2 to 150 fragments; at a head, reaching a
    tail, in the interior): flip_rounds(min_score=20) restores every chromosome's order and every fragment's orientation, and every
    kept round raises logL.  min_score must sit between two figures of the windowed restatement on the list this test scores, and
    the test asserts that first, on the engine's own list (seed 2024), and prints both.  On that list as tests/sim_reference.simulate
    restates it (203,471 entries, 696,080 contacts; the engine's list but for at most 5 background chunks whose draws may round
    differently) the largest of the 6,888 runs of 2-8 fragments of the TRUE layout scores 1.4 (2 above 0), the smallest planted block
    gains 427.2 (the seven: 518.0, 997.7, 6,217.3, 427.2, 7,270.8, 578.5, 575.5), and the rounds driven by the restatement alone
    restore all seven in one round.  On contacts drawn by numpy (seed 5; tests/test_flips_cpu.py) the two figures are 2.1 and 372.8."""
    e, s = simulated()
    try:
        spurious, gains = spurious_and_planted(e, s)
        print("largest spurious flip %.1f, planted gains %s" % (spurious, np.round(gains, 1).tolist()))
        assert spurious < 20.0 < gains.min(), (spurious, gains)
        bad, _, _ = planted(s)
        with pytest.raises(AssertionError):
            assert_true_chromosomes_and_orientations(bad, s)
        e.upload_frags(bad)
        rec = flips.flip_rounds(e, max_frags=8, junction_below=0.0, max_units=3, min_score=20.0)
        got = e.download_frags()
    finally:
        e.close()
    kept = [r["logL"] for r in rec if r["kept"]]
    assert len(kept) >= 2 and all(b > a for a, b in zip(kept, kept[1:])), rec
    assert_true_chromosomes_and_orientations(got, s)


def test_scaffold_with_flips_repairs_a_wrongly_oriented_piece():
    """scaffold() alone keeps the orientation a small piece was joined in; with flip_max_frags set, the flip rounds behind it (their
    marks include the joins scaffold made) turn it round.  The default leaves scaffold() as it was: no flip rows."""
    e, s = simulated()
    try:
        chroms = list(LR.contig_lists(s).values())
        c0 = chroms[0]
        wrong = c0[:200] + [(f, -o) for f, o in reversed(c0[200:204])] + c0[204:]
        start = LR.layout(s["len_bp"], [wrong] + chroms[1:])
        e.upload_frags(start)
        plain = scaffold.scaffold(e, rounds=5)
        got_plain = e.download_frags()
        e.upload_frags(start)
        rec = scaffold.scaffold(e, rounds=5, flip_max_frags=8, flip_min_score=20.0)
        got = e.download_frags()
    finally:
        e.close()
    assert len(rec) > len(plain) and rec[-1]["kept"] == 1 and rec[-1]["logL"] > plain[-1]["logL"]
    with pytest.raises(AssertionError):
        assert_true_chromosomes_and_orientations(got_plain, s)
    assert_true_chromosomes_and_orientations(got, s)


def test_run_flip_and_flips_write_their_tables():
    """--flip writes its rounds, --flips the score table of the tilings of the final layout."""
    P = synth.make_problem(n_bins=300, nnz=30000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    with tempfile.TemporaryDirectory() as d:
        data = os.path.join(d, "data")
        synth.write_dataset(P, data)
        out = os.path.join(d, "out")
        cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
               "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--flip", "--flips", "--flip-max-frags", "3",
               "--no-fit", "--param", *[str(float(x)) for x in synth.make_param_simu(fact=300.0, v_inter=0.02)]]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(os.path.join(out, "flip.tsv")).read().splitlines()
        assert lines[0].split("\t") == list(flips.ROUND_COLUMNS) and lines[1].split("\t")[0] == "0"
        lines = open(os.path.join(out, "flips.tsv")).read().splitlines()
        assert lines[0].split("\t") == list(flips.COLUMNS)
        rows = [l.split("\t") for l in lines[1:]]
        assert len(rows) > 0 and all(1 <= int(x[5]) <= 3 for x in rows)
        assert len({(x[0], x[1]) for x in rows}) == len(rows)
