"""graal_junction_bootstrap on the GPU: the data's own scores word for word those of graal_junction_scores, every replicate equal to the
numpy restatement (tests/junction_boot_reference.py) outside the cells a near-boundary draw excuses, the statistics exactly those of the
returned matrix, deterministic and independent of n_rep and of the batching, refused where graal_junction_scores is, free of side
effects on a run, and sensible on simulated data with planted misjoins."""
import ctypes
import functools
import mmap
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from graal_amd import em, junctions, synth
from graal_amd.lib import Engine, GraalError, JUNCTION_VALID
from tests import junction_boot_reference as BR
from tests.test_junctions_gpu import _layout, engine_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [pytest.param(*c, id="%s-%d-%d" % c) for c in BR.SMALL_CASES]


def tol(A):
    return 1e-9 * np.asarray(A, np.float64) + 1           # tests/test_layout_scores_midsize_gpu.py's bound, in Q


@functools.lru_cache(maxsize=None)
def gpu(name, quirk, seed):
    """One engine per case: graal_junction_scores, then the bootstrap of N_REP replicates twice, of 5, without the matrix, and at a
    threshold taken from the matrix."""
    e = engine_for(BR.small_case(name), quirk=quirk)
    try:
        out = {"scores": e.junction_scores_q()}
        out["full"] = e.junction_bootstrap_q(seed, BR.N_REP, 0, replicates=True)
        out["again"] = e.junction_bootstrap_q(seed, BR.N_REP, 0, replicates=True)
        out["five"] = e.junction_bootstrap_q(seed, 5, 0, replicates=True)
        out["plain"] = e.junction_bootstrap_q(seed, BR.N_REP, 0)
        ok = np.nonzero(out["full"]["status"] == JUNCTION_VALID)[0]
        out["threshold"] = int(out["full"]["q_rep"][3, ok[len(ok) // 2]])
        out["at_threshold"] = e.junction_bootstrap_q(seed, BR.N_REP, out["threshold"], replicates=True)
        out["other_seed"] = e.junction_bootstrap_q(seed + 1, 5, 0, replicates=True)
        out["scores_after"] = e.junction_scores_q()
    finally:
        e.close()
    return out


@pytest.mark.parametrize("name,quirk,seed", CASES)
def test_data_scores_are_junction_scores(name, quirk, seed):
    g = gpu(name, quirk, seed)
    q, st = g["scores"]
    for k in ("full", "five", "plain", "at_threshold"):
        assert np.array_equal(g[k]["q"], q) and np.array_equal(g[k]["status"], st), k
    assert np.array_equal(g["scores_after"][0], q) and np.array_equal(g["scores_after"][1], st)
    assert (st == JUNCTION_VALID).sum() >= 10


@pytest.mark.parametrize("name,quirk,seed", CASES)
def test_replicates_equal_restatement(name, quirk, seed):
    g = gpu(name, quirk, seed)["full"]
    B = BR.small_boot(name, quirk)
    J, A, flagged, nf = BR.small_replicates(name, quirk, seed)
    assert np.array_equal(g["status"], B.status) and not nf.any()
    ok = g["status"] == JUNCTION_VALID
    rep = g["q_rep"][list(BR.REF_REPS)]
    assert rep.shape == J.shape and not rep[:, ~ok].any()
    cells = ok[None, :] & ~flagged
    assert cells.sum() >= 0.98 * ok.sum() * len(BR.REF_REPS)
    excess = np.abs(rep - J)[cells] / tol(A[cells])
    print("%s quirk %d: %d cells, %d flagged, largest |q_rep - J*| / tolerance %.3e" % (name, quirk, cells.sum(), (flagged & ok).sum(),
                                                                                      float(excess.max())))
    assert (excess <= 1).all(), int((excess > 1).sum())
    # the replicates differ from the data's own scores and from each other: the draws are in them
    assert (rep[0][ok] != g["q"][ok]).mean() > 0.9 and (rep[0][ok] != rep[1][ok]).mean() > 0.9
    # both branches of the sampler and the fill value, each under at least three valid junctions
    classes = {"inversion": B.ob < 10, "ptrs": np.isin(B.ob, BR.PLANTED), "fill": B.ob != np.rint(B.ob)}
    for k, m in classes.items():
        assert m.any() and (B.straddle(np.ones(len(B.ob)), select=m)[ok] > 0).sum() >= 3, k
    assert classes["fill"].sum() == 1 and classes["ptrs"].sum() >= len(BR.PLANTED)


@pytest.mark.parametrize("name,quirk,seed", CASES)
def test_statistics_are_those_of_the_matrix(name, quirk, seed):
    G = gpu(name, quirk, seed)
    for k, thr in (("full", 0), ("at_threshold", G["threshold"]), ("five", 0)):
        g = G[k]
        ok = g["status"] == JUNCTION_VALID
        rep = g["q_rep"]
        assert np.array_equal(g["support"], np.where(ok, (rep > thr).sum(axis=0), 0)), k
        assert np.array_equal(g["q_sum"], np.where(ok, rep.sum(axis=0), 0)), k
        assert np.array_equal(g["q_min"], np.where(ok, rep.min(axis=0), 0)), k
        assert np.array_equal(g["q_max"], np.where(ok, rep.max(axis=0), 0)), k
        assert g["support"].dtype == np.int32 and (g["q_min"][ok] < g["q_max"][ok]).all()


@pytest.mark.parametrize("name,quirk,seed", CASES)
def test_deterministic_whatever_n_rep_and_threshold(name, quirk, seed):
    G = gpu(name, quirk, seed)
    full = G["full"]
    for k in full:
        assert np.array_equal(full[k], G["again"][k]), k
    for k in ("q", "status", "support", "q_sum", "q_min", "q_max"):
        assert np.array_equal(full[k], G["plain"][k]), k
    assert "q_rep" not in G["plain"]
    # N_REP spans three batches, the last one short: its first five rows are the call of five
    assert BR.N_REP > 2 * 64 and BR.N_REP % 64 != 0
    assert np.array_equal(G["five"]["q_rep"], full["q_rep"][:5])
    assert np.array_equal(G["at_threshold"]["q_rep"], full["q_rep"])
    ok = full["status"] == JUNCTION_VALID
    assert (G["other_seed"]["q_rep"][:, ok] != G["five"]["q_rep"][:, ok]).mean() > 0.9
    # a threshold at one replicate's value moves the support by exactly the replicates between 0 and it
    thr = G["threshold"]
    lo, hi = min(0, thr), max(0, thr)
    between = ((full["q_rep"] > lo) & (full["q_rep"] <= hi)).sum(axis=0) * (1 if thr > 0 else -1)
    assert thr != 0 and np.array_equal(full["support"] - G["at_threshold"]["support"], np.where(ok, between, 0))
    assert (full["support"] != G["at_threshold"]["support"]).any()


def test_float_columns():
    name, quirk, seed = BR.SMALL_CASES[0]
    G = gpu(name, quirk, seed)["five"]
    e = engine_for(BR.small_case(name), quirk=quirk)
    try:
        f = e.junction_bootstrap(seed, 5, replicates=True)
        t = junctions.support_table(e, seed, 5)
        J, _ = e.junction_scores()
    finally:
        e.close()
    ok = G["status"] == JUNCTION_VALID
    Qs = float(1 << 30)
    assert np.array_equal(f["status"], G["status"]) and np.isnan(f["support"][~ok]).all() and np.isnan(f["replicates"][:, ~ok]).all()
    assert np.array_equal(f["support"][ok], G["support"][ok] / 5.0) and ((f["support"][ok] >= 0) & (f["support"][ok] <= 1)).all()
    assert np.array_equal(f["mean"][ok], G["q_sum"][ok] / 5.0 / Qs) and np.array_equal(f["min"][ok], G["q_min"][ok] / Qs)
    assert np.array_equal(f["max"][ok], G["q_max"][ok] / Qs) and np.array_equal(f["replicates"][:, ok], G["q_rep"][:, ok] / Qs)
    assert np.array_equal(f["J"][ok], J[ok])
    assert tuple(t) == junctions.SUPPORT_COLUMNS and len(t["support"]) == ok.sum()
    assert np.array_equal(t["support"], f["support"][t["left_frag"]]) and np.array_equal(t["score"], J[t["left_frag"]])


def test_no_side_effect_on_a_run():
    """run_em with junction_bootstrap_q() called at the end of every cycle and in the middle of one gives the same accepted moves and
    likelihoods (tests/test_junctions_gpu.py's pattern)."""
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
                calls.append(smp.engine.junction_bootstrap_q(3, 5, 0, replicates=True))

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs)))
        smp.free_gpu()
        assert (len(calls) >= 3) == call
    (m0, l0, c0), (m1, l1, c1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1)


def test_refusals():
    name, quirk, seed = BR.SMALL_CASES[2]
    P = BR.small_case(name)
    want = gpu(name, quirk, seed)["five"]
    e = engine_for(P)
    try:
        seg = mmap.mmap(-1, max(e.exchange_bytes(2), mmap.PAGESIZE))   # (rank 0 of two: a world of one has no exchange)
        e.attach_exchange(seg, 0, 2, 0)
        with pytest.raises(GraalError, match=r"one rank.*code 3\)"):
            e.junction_bootstrap_q(seed, 5)
        e.detach_exchange()
        for n_rep in (0, 1025, -1):
            with pytest.raises(GraalError, match=r"code 1\)"):
                e.junction_bootstrap_q(seed, n_rep, 0, replicates=True)
        n = e.n
        i64 = lambda: np.zeros(n, np.int64)
        q, s, lo, hi = i64(), i64(), i64(), i64()
        st = np.zeros(n, np.uint8)
        p64 = ctypes.POINTER(ctypes.c_int64)
        rc = e._L.graal_junction_bootstrap(e._h, ctypes.c_uint64(seed), 5, 0, q.ctypes.data_as(p64), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                           None, s.ctypes.data_as(p64), lo.ctypes.data_as(p64), hi.ctypes.data_as(p64), None)
        assert rc == 1 and not q.any() and not s.any()
        got = e.junction_bootstrap_q(seed, 5, 0, replicates=True)       # the engine works afterwards
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.junction_bootstrap_q(1, 5)
    finally:
        e.close()


def test_simulated_genome_supports_its_joins_more_than_planted_misjoins():
    """tests/test_junctions_gpu.py's simulated 1,000-bin genome with the second halves of contigs 0 and 1 swapped, 64 replicates: both
    planted misjoins have less support than the true joins have on average, and a junction whose smallest replicate is positive is
    supported by all 64.  Measured (printed below; one MI355X, resampling seed 77): the true joins' mean support 0.9994, the weakest
    of them 50 / 64 (smallest replicate -35.6 log units); the two misjoins, J = -236.0 and -160.5, have support 0 / 64 (largest
    replicates -215.3 and -139.5)."""
    R = 64
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
        contigs = []
        for cid in np.unique(s["id_c"]):
            m = np.nonzero(s["id_c"] == cid)[0]
            contigs.append([(int(f), int(s["ori"][f])) for f in m[np.argsort(s["pos"][m])]])
        a, b = contigs[0], contigs[1]
        ha, hb = len(a) // 2, len(b) // 2
        contigs[0], contigs[1] = a[:ha] + b[hb:], b[:hb] + a[ha:]
        bad = {a[ha - 1][0], b[hb - 1][0]}
        e.upload_frags(_layout(s["len_bp"], contigs))
        g = e.junction_bootstrap_q(77, R, 0, replicates=True)
    finally:
        e.close()
    ok = g["status"] == JUNCTION_VALID
    mis = np.array(sorted(bad))
    true = np.array([f for f in np.nonzero(ok)[0] if f not in bad])
    assert ok[mis].all() and len(true) == 1000 - 3 - 2
    Qs = float(1 << 30)
    print("true joins: mean support %.4f, smallest %d / %d, smallest replicate %.1f; misjoins: support %s / %d, J %s, largest replicates %s"
          % (g["support"][true].mean() / R, g["support"][true].min(), R, g["q_min"][true].min() / Qs, g["support"][mis].tolist(), R,
             (g["q"][mis] / Qs).round(1).tolist(), (g["q_max"][mis] / Qs).round(1).tolist()))
    assert (g["support"][mis] < g["support"][true].mean()).all()
    sure = ok & (g["q_min"] > 0)
    assert sure.sum() >= 3 and (g["support"][sure] == R).all()
    assert (g["support"][ok & (g["q_max"] <= 0)] == 0).all()


def test_run_writes_junction_support_tsv():
    """The rows are support_table's of the layout the run ended in (its fragments, orientations and order are in the rows themselves),
    on a sampler built from the same dataset the way graal_amd.run builds its own, with the run's --seed for the resampling."""
    from graal_amd import pyramid as pyr
    from graal_amd.sampler import sampler
    P = synth.make_problem(n_bins=300, nnz=3000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    par = synth.make_param_simu(fact=300.0, v_inter=0.02)
    with tempfile.TemporaryDirectory() as d:
        data, out = os.path.join(d, "data"), os.path.join(d, "out")
        synth.write_dataset(P, data)
        cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
               "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--junctions", "--junction-support", "16",
               "--no-fit", "--param", *[str(float(x)) for x in par]]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(os.path.join(out, "junction_support.tsv")).read().splitlines()
        plain = open(os.path.join(out, "junctions.tsv")).read().splitlines()
        root = os.path.join(data, "pyramids", "pyramid_1_thresh_auto")
        inp = pyr.simulation_inputs(pyr.Pyramid(root, 1), 0, candidates_blacklist=[0], allow_repeats=False)
    assert lines[0].split("\t") == list(junctions.SUPPORT_COLUMNS)
    rows = [l.split("\t") for l in lines[1:]]
    nc = len(junctions.COLUMNS)
    assert len(rows) == len(plain) - 1 > 0 and [x[:nc] for x in rows] == [l.split("\t") for l in plain[1:]]
    left = np.array([int(x[2]) for x in rows]); right = np.array([int(x[3]) for x in rows])
    n = int(inp["n_frags"])
    members = {}
    for x in rows:
        members.setdefault(int(x[0]), []).append(x)
    contigs = [[(int(x[2]), int(x[4])) for x in m] + [(int(m[-1][3]), int(m[-1][5]))] for _, m in sorted(members.items())]
    in_rows = set(left.tolist()) | set(right.tolist())
    contigs += [[(f, 1)] for f in range(n) if f not in in_rows]     # (fragments without a scored junction: alone, they change no score)
    smp = sampler(True, inp["S_o_A_frags"], inp["collector_id_repeats"], inp["frag_dispatcher"], inp["id_frag_duplicated"],
                  inp["id_frags_blacklisted"], inp["n_frags"], inp["n_new_frags"], inp["init_n_sub_frags"], inp["n_new_sub_frags"],
                  None, inp["hic_matrix_sub_sampled"], inp["np_sub_frags_len_bp"], inp["np_sub_frags_id"], inp["np_sub_frags_accu"],
                  inp["mean_squared_frags_per_bin"], inp["norm_vect_accu"], inp["S_o_A_sub_frags"], inp["hic_matrix"],
                  inp["mean_value_trans"], 1, False, None, device=0, rng=np.random.RandomState(3), reference_arithmetic="exact")
    try:
        smp.set_param_simu(np.asarray(par, dtype=np.float32))
        smp.engine.upload_frags(_layout(np.asarray(inp["S_o_A_frags"]["len_bp"]), contigs))
        t = junctions.support_table(smp, 3, 16)
    finally:
        smp.free_gpu()
    assert np.array_equal(t["left_frag"], left) and np.array_equal(t["right_frag"], right)
    for j, c in enumerate(junctions.SUPPORT_COLUMNS[nc - 1:]):
        got = np.array([float(x[nc - 1 + j]) for x in rows])
        assert np.array_equal(got, t[c], equal_nan=True), c
    assert ((t["support"] >= 0) & (t["support"] <= 1)).all() and (t["support"] * 16 == np.rint(t["support"] * 16)).all()
