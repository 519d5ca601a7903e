"""graal_junction_scores on the GPU: equal to the numpy restatement (tests/junction_reference.py), consistent with the engine's own
candidate deltas and full evaluations, deterministic, right on simulated data with planted misjoins, and free of side effects on a run."""
import mmap
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from graal_amd import em, junctions, synth
from graal_amd.lib import Engine, GraalError, JUNCTION_CIRCULAR, JUNCTION_VALID
from oracle.sparse_numpy import SparseScorer
from tests import junction_reference as JR

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


@pytest.mark.parametrize("name,quirk", [("sub3", False), ("sub3", True), ("sub1", False), ("circ", False)])
def test_equals_reference(name, quirk):
    P = JR.case(name)
    e = engine_for(P, quirk=quirk)
    try:
        q, st = e.junction_scores_q()
    finally:
        e.close()
    J, st_ref, A = JR.reference(P, quirk=quirk)
    assert np.array_equal(st, st_ref)
    ok = st == JUNCTION_VALID
    assert ok.sum() >= 10 and (q[~ok] == 0).all()
    assert np.all(np.abs(q[ok] - J[ok]) <= 1e-9 * A[ok] + 1), np.max(np.abs(q[ok] - J[ok]))
    if name == "circ":
        assert (st[P["S_o_A_frags"]["circ"] == 1] == JUNCTION_CIRCULAR).all()


@pytest.mark.parametrize("name", ["sub3", "sub1"])
def test_contig_ends_equal_minus_eject_delta(name):
    """A fragment at either end of a contig has one junction; ejecting it (candidate 0) is cutting there: J = -delta in exact arithmetic."""
    P = JR.case(name)
    s = P["S_o_A_frags"]
    e = engine_for(P)
    try:
        J, st = e.junction_scores()
        max_id = e.relabel_contigs()
        checked = 0
        for f in range(len(s["pos"])):
            if s["l_cont"][f] < 2 or (s["prev"][f] != -1 and s["next"][f] != -1):
                continue
            left = f if s["next"][f] != -1 else int(s["prev"][f])
            fb = int(s["next"][f]) if s["next"][f] != -1 else int(s["prev"][f])
            d = e.eval_candidates(f, [fb], max_id)[0, 0]
            assert st[left] == JUNCTION_VALID
            assert abs(J[left] + d) <= 1e-7 * max(1.0, abs(d)), (f, J[left], d)
            checked += 1
        assert checked >= 4
    finally:
        e.close()


@pytest.mark.parametrize("name", ["sub3", "sub1"])
def test_inner_junctions_equal_full_evaluation_difference(name):
    """J = eval_full(layout) - eval_full(cut layout), within the float32 re-centring noise of the part that moves (measured with the
    sparse scorer: the cut priced with and without re-centring)."""
    P = JR.case(name)
    s = {k: np.ascontiguousarray(v, dtype=np.int32) for k, v in P["S_o_A_frags"].items()}
    sp = SparseScorer(P["coo_row"], P["coo_col"], P["coo_val"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["param_simu"])
    e = engine_for(P)
    try:
        J, st = e.junction_scores()
        e.relabel_contigs()
        base = e.eval_full()
        inner = [f for f in np.nonzero(st == JUNCTION_VALID)[0] if s["prev"][f] != -1 and s["next"][s["next"][f]] != -1]
        assert len(inner) >= 5
        for f in inner[:: max(1, len(inner) // 6)]:
            cut = JR.cut_layout(s, int(f))
            noise = abs(sp.full(cut) - sp.full(JR.cut_layout(s, int(f), recentre=False)))
            e.upload_frags(cut)
            e.relabel_contigs()
            want = base - e.eval_full()
            assert abs(J[f] - want) <= 1.5 * noise + 1e-6, (f, J[f], want, noise)
        e.upload_frags(s)
    finally:
        e.close()


def test_deterministic_and_round_trip():
    P = JR.case("sub3")
    e = engine_for(P)
    try:
        a = e.junction_scores_q()
        b = e.junction_scores_q()
        soa = e.download_frags()
        e.upload_frags(soa)
        c = e.junction_scores_q()
    finally:
        e.close()
    for x in (b, c):
        assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1])


def _layout(lens, contigs):
    """Fragment fields of a layout given as lists of (fragment, orientation) per contig."""
    n = len(lens)
    s = {k: np.zeros(n, np.int32) for k in ("pos", "id_c", "start_bp", "len_bp", "circ", "id", "prev", "next", "l_cont", "l_cont_bp", "ori",
                                            "rep", "activ", "id_d")}
    s["len_bp"][:] = lens; s["id"][:] = np.arange(n); s["id_d"][:] = np.arange(n); s["activ"][:] = 1
    for c, frags in enumerate(contigs):
        run = 0
        tot = int(sum(lens[f] for f, _ in frags))
        for p, (f, o) in enumerate(frags):
            s["pos"][f] = p; s["id_c"][f] = c; s["start_bp"][f] = run; s["ori"][f] = o
            s["prev"][f] = frags[p - 1][0] if p > 0 else -1
            s["next"][f] = frags[p + 1][0] if p + 1 < len(frags) else -1
            s["l_cont"][f] = len(frags); s["l_cont_bp"][f] = tot
            run += int(lens[f])
    return s


def test_simulated_genome_supports_its_joins_and_not_planted_misjoins():
    par = synth.make_param_simu(fact=300.0, v_inter=0.02)
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(5, 3, 2), param=par)
    s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.set_params(par)
        e.upload_frags(s)
        r, c, v = e.simulate_contacts(2024)
        e.upload_contacts(r, c, v)
        J, st = e.junction_scores()
        ok = st == JUNCTION_VALID
        assert ok.sum() == int((s["next"] != -1).sum()) and np.all(J[ok] > 0), np.nanmin(J)
        # two planted misjoins: the second halves of contigs 0 and 1 swapped
        contigs = []
        for cid in np.unique(s["id_c"]):
            m = np.nonzero(s["id_c"] == cid)[0]
            contigs.append([(int(f), int(s["ori"][f])) for f in m[np.argsort(s["pos"][m])]])
        a, b = contigs[0], contigs[1]
        ha, hb = len(a) // 2, len(b) // 2
        contigs[0], contigs[1] = a[:ha] + b[hb:], b[:hb] + a[ha:]
        bad = {a[ha - 1][0], b[hb - 1][0]}
        e.upload_frags(_layout(s["len_bp"], contigs))
        J2, st2 = e.junction_scores()
        ok2 = st2 == JUNCTION_VALID
        mis = np.array(sorted(bad))
        true = np.array([f for f in np.nonzero(ok2)[0] if f not in bad])
        assert (st2[mis] == JUNCTION_VALID).all()
        assert J2[mis].max() < J2[true].min(), (J2[mis], J2[true].min())
    finally:
        e.close()


def _sampler(P, rng):
    from tests.test_sampler_gpu import make_gpu_sampler
    return make_gpu_sampler(P, rng, reference_arithmetic="exact")


def test_no_side_effect_on_a_run():
    """run_em with junction_scores() called at the end of every cycle and in the middle of one gives the same accepted moves and likelihoods."""
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
                smp.engine.junction_scores()

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs)))
        smp.free_gpu()
    (m0, l0, c0), (m1, l1, c1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1)


def test_repeats_and_ranks_refused():
    P = JR.case("sub1")
    e = engine_for(P)
    try:
        seg = mmap.mmap(-1, max(e.exchange_bytes(2), mmap.PAGESIZE))   # (rank 0 of two: a world of one has no exchange)
        e.attach_exchange(seg, 0, 2, 0)
        with pytest.raises(GraalError, match="one rank"):
            e.junction_scores()
        e.detach_exchange()
        e.junction_scores()
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.junction_scores()
    finally:
        e.close()


def test_run_writes_junctions_tsv():
    P = synth.make_problem(n_bins=300, nnz=3000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    with tempfile.TemporaryDirectory() as d:
        data, out = os.path.join(d, "data"), os.path.join(d, "out")
        synth.write_dataset(P, data)
        cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
               "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--junctions",
               "--no-fit", "--param", *[str(float(x)) for x in synth.make_param_simu(fact=300.0, v_inter=0.02)]]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(os.path.join(out, "junctions.tsv")).read().splitlines()
        assert lines[0].split("\t") == list(junctions.COLUMNS)
        rows = [l.split("\t") for l in lines[1:]]
        import re
        n_contigs = int(re.search(r"steps in .*?: (\d+) contigs", r.stdout).group(1))
        assert 0 < len(rows) <= 300 - n_contigs     # (one per join of a linear contig; a ring's joins have no row)
        contig = np.array([int(x[0]) for x in rows]); pos = np.array([int(x[1]) for x in rows])
        assert np.all(np.diff(contig * 10**6 + pos) > 0)
        assert all(x[-1] != "nan" for x in rows)
