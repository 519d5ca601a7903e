"""graal_simulate_contacts on the GPU: equal to the numpy restatement (tests/sim_reference.py), deterministic, model-faithful at C5 size,
and usable end to end (likelihood, Rippe fit, the simulate -> run command line)."""
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

from graal_amd import rippe_fit, synth
from graal_amd.lib import Engine, GraalError, Q_SCALE
from graal_amd.simulate import simulate_contacts, simulate_problem
from tests import sim_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name):
    par = synth.make_param_simu(fact=2000.0, v_inter=0.05)
    if name == "sub3":
        P = synth.make_problem(n_bins=90, nnz=300, n_sub=3, seed=21, contig_weights=(5, 3, 2), mean_len_bp=1500.0, accu=("random", 1, 4), param=par)
        P["S_o_A_frags"] = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
        P["S_o_A_frags"]["ori"][::4] = -1                 # reversed bins
    elif name == "sub1":
        P = synth.make_problem(n_bins=400, nnz=300, n_sub=1, seed=22, contig_weights=(4, 3, 3), param=par)
    elif name == "chunks":                                # S > 2 * 4096: background chunks k = 0, 1, 2 and their edges
        par = synth.make_param_simu(fact=30.0, v_inter=2e-4)
        P = synth.make_problem(n_bins=9000, nnz=500, n_sub=1, seed=31, contig_weights=(4, 3, 3), accu=("random", 1, 3), param=par)
        P["S_o_A_frags"] = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
        P["S_o_A_frags"]["ori"][::5] = -1
    else:                                                 # circular contig, RF counts > 1
        P = synth.make_problem(n_bins=80, nnz=300, n_sub=3, seed=23, contig_weights=(2, 1), mean_len_bp=1500.0, accu=9, param=par)
        s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
        s["circ"][s["id_c"] == s["id_c"].min()] = 1
        P["S_o_A_frags"] = s
    return P, par


@pytest.mark.parametrize("name", ["sub3", "sub1", "circ", "chunks"])
def test_equals_reference(name):
    P, par = _case(name)
    got = simulate_contacts(P, 77)
    want = R.simulate(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"], par,
                      P["S_o_A_frags"], 77)
    diff, unexplained = R.compare(got, want[:3], want[3], want[4])
    nnz = len(want[0])
    assert nnz > 500
    assert unexplained == [], unexplained[:10]
    assert len(diff) <= math.ceil(1e-4 * nnz), (len(diff), nnz)
    _well_formed(*got, P["init_n_sub_frags"])            # (R.compare ignores order and duplicates)
    if name == "chunks":
        S = P["init_n_sub_frags"]
        assert S > 2 * R.CHUNK
        k = got[1] // R.CHUNK
        assert all((k == j).sum() > 1000 for j in range(3))
        # columns at both edges of every chunk boundary, in rows on either side of it
        for edge in (R.CHUNK, 2 * R.CHUNK):
            assert ((got[1] == edge - 1) | (got[1] == edge)).any()


def _well_formed(r, c, v, S):
    assert np.all(r < c) and np.all(v > 0) and np.all(r >= 0) and np.all(c < S)
    k = r.astype(np.int64) * S + c
    assert np.all(np.diff(k) > 0)


def test_deterministic_and_seeded():
    P, par = _case("sub3")
    a = simulate_contacts(P, 5)
    b = simulate_contacts(P, 5)
    c = simulate_contacts(P, 6)
    for x in (a, b, c):
        _well_formed(*x, P["init_n_sub_frags"])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not (len(a[0]) == len(c[0]) and all(np.array_equal(x, y) for x, y in zip(a, c)))


def test_repeats_unsupported():
    from tests.test_repeats_gpu import engine_with_repeats
    P, par = _case("sub1")
    P = synth.with_dense(synth.add_repeats(P, [3, 40], 2))
    e = engine_with_repeats(P, P["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match="not supported"):
            e.simulate_contacts(1)
    finally:
        e.close()


def test_c5_layout_mass_and_distance_classes():
    par = synth.make_param_simu()
    P = synth.make_problem(n_bins=50000, nnz=1000, n_sub=1, seed=20141217, param=par)   # bench.py's C5 layout (contacts not needed)
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.set_params(par)
        e.upload_frags(P["S_o_A_frags"])
        r, c, v = e.simulate_contacts(2016)
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            e.simulate_contacts(2016)
            times.append(time.perf_counter() - t0)
        print("C5 simulation: %d contacts, sum %d; %.1f ms per simulation incl. the copy to the host (best of 3)"
              % (len(v), int(v.sum()), 1e3 * min(times)))
        _well_formed(r, c, v, P["init_n_sub_frags"])
        # the expected mass of all pixels, from the engine's own full likelihood (q[1] = -sum of lambda)
        e.upload_contacts(r, c, v)
        e.relabel_contigs()
        lam_sum = -float(e.eval_full_q()[1]) / Q_SCALE
    finally:
        e.close()
    tot = float(v.sum(dtype=np.int64))
    assert abs(tot - lam_sum) <= 5 * math.sqrt(lam_sum), (tot, lam_sum)
    # per distance class (offset k in the genome order, cis): observed vs expected sums
    S = P["S_o_A_frags"]
    centre = (S["start_bp"].astype(np.float32) / np.float32(1000) + (S["len_bp"].astype(np.float32) / np.float32(1000)) / np.float32(2)).astype(np.float32)
    key = r.astype(np.int64) * len(centre) + c
    kv = dict(zip(key.tolist(), v.tolist()))
    for k in (1, 2, 10, 100, 1000):
        i = np.arange(len(centre) - k)
        j = i + k
        cis = S["id_c"][i] == S["id_c"][j]
        i, j = i[cis], j[cis]
        lam = R.pair_lambda((centre, S["id_c"].astype(np.int64), np.ones(len(centre), np.int64), np.full(len(centre), -1)), i, j, 1.0, par)
        obs = sum(kv.get(x, 0) for x in (i * len(centre) + j).tolist())
        assert abs(obs - lam.sum()) <= 5 * math.sqrt(lam.sum()) + 1, (k, obs, lam.sum())
    # trans
    trans = S["id_c"][r] != S["id_c"][c]
    n_c = np.bincount(S["id_c"]).astype(np.float64)
    n_trans = (float(n_c.sum()) ** 2 - float((n_c ** 2).sum())) / 2.0
    want = float(par[7]) * n_trans
    assert abs(float(v[trans].sum()) - want) <= 5 * math.sqrt(want)


def _genome_1000():
    par = synth.make_param_simu(fact=1e4, v_inter=1e-3)
    P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(5, 3, 2), param=par)
    return simulate_problem(P, 1), par


def test_end_to_end_likelihood_and_fit():
    Q, par = _genome_1000()
    S = Q["S_o_A_frags"]
    n = Q["n_frags"]
    boom = {k: np.array(v) for k, v in S.items()}         # the exploded genome: every fragment its own contig
    boom.update(id_c=np.arange(n, dtype=np.int32), pos=np.zeros(n, np.int32), start_bp=np.zeros(n, np.int32), circ=np.zeros(n, np.int32),
                prev=np.full(n, -1, np.int32), next=np.full(n, -1, np.int32), l_cont=np.ones(n, np.int32), l_cont_bp=boom["len_bp"].copy(),
                ori=np.ones(n, np.int32))
    e = Engine(0)
    try:
        e.upload_subfrags(Q["np_sub_frags_id"], Q["np_sub_frags_len_bp"], Q["np_sub_frags_accu"], Q["init_n_sub_frags"],
                          Q["mean_squared_frags_per_bin"])
        e.upload_contacts(Q["coo_row"], Q["coo_col"], Q["coo_val"])
        e.set_params(par)
        logl = []
        for s in (S, boom):
            e.upload_frags(s)
            e.relabel_contigs()
            logl.append(e.eval_full())
    finally:
        e.close()
    assert logl[0] > logl[1], logl
    # the Rippe fit of the simulated contacts against the same fit of the model's expected histogram (the estimator's own bias, ~0.045
    # in the slope on this genome, cancels): slope within 0.05, amplitude within 10 %
    size_bin = float(np.mean(S["len_bp"])) / 1000.0
    max_dist = float(S["l_cont_bp"][S["start_bp"] == 0].mean()) / 1000.0
    bins = np.arange(size_bin, max_dist + size_bin, size_bin)
    a, b, lam = R.expected_lambda_matrix(Q["np_sub_frags_id"], Q["np_sub_frags_len_bp"], Q["np_sub_frags_accu"],
                                         Q["mean_squared_frags_per_bin"], par, S)
    pe, _ = rippe_fit.estimate_param_rippe(rippe_fit.mean_contacts_per_bin(S, (a, b, lam), bins, max_dist, size_bin), bins)
    ps, _ = rippe_fit.estimate_param_rippe(rippe_fit.mean_contacts_per_bin(S, (Q["coo_row"], Q["coo_col"], Q["coo_val"]), bins, max_dist,
                                                                           size_bin), bins)
    x0 = bins[len(bins) // 4]
    amp = rippe_fit.peval(x0, [ps[0], ps[1], ps[2], ps[4]]) / rippe_fit.peval(x0, [pe[0], pe[1], pe[2], pe[4]])
    assert abs(ps[2] - pe[2]) <= 0.05 and abs(amp - 1.0) <= 0.10, (ps, pe, amp)


def test_cli_simulate_then_run():
    P = synth.make_problem(n_bins=1000, nnz=3000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    env = dict(os.environ, PYTHONPATH=ROOT)
    with tempfile.TemporaryDirectory() as d:
        src, sim, out = (os.path.join(d, x) for x in ("src", "sim", "out"))
        synth.write_dataset(P, src)
        cmd = [sys.executable, "-m", "graal_amd.simulate", "--dataset", src, "--seed", "3", "--out", sim]
        r = subprocess.run(["timeout", "-k", "10", "120"] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", sim, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
               "--seed", "1", "--out", out]
        r = subprocess.run(["timeout", "-k", "10", "240"] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        print(r.stdout[-600:])


def test_pyramid_problem_feeds_the_sampler(tmp_path):
    """A pyramid.simulation_inputs dict through simulate_problem: a sampler built from the result scores the SIMULATED data (its full
    likelihood equals the engine's on the simulated list), not the dataset's."""
    from graal_amd.sampler import sampler
    from tests.test_simulate_cpu import pyramid_problem
    inp = pyramid_problem(str(tmp_path))
    out = simulate_problem(inp, 8)
    r, c, v = simulate_contacts(inp, 8)

    def full_logl(P):
        smp = sampler(True, P["S_o_A_frags"], P["collector_id_repeats"], P["frag_dispatcher"], P["id_frag_duplicated"],
                      P["id_frags_blacklisted"], P["n_frags"], P["n_new_frags"], P["init_n_sub_frags"], P["n_new_sub_frags"], None,
                      P["hic_matrix_sub_sampled"], P["np_sub_frags_len_bp"], P["np_sub_frags_id"], P["np_sub_frags_accu"],
                      P["mean_squared_frags_per_bin"], P["norm_vect_accu"], P["S_o_A_sub_frags"], P["hic_matrix"], P["mean_value_trans"],
                      1, False, None, rng=np.random.RandomState(0), param_simu=P["param_simu"], reference_arithmetic="exact")
        try:
            return smp.eval_likelihood()
        finally:
            smp.free_gpu()

    e = Engine(0)
    try:
        e.upload_subfrags(inp["np_sub_frags_id"], inp["np_sub_frags_len_bp"], inp["np_sub_frags_accu"], inp["init_n_sub_frags"],
                          inp["mean_squared_frags_per_bin"])
        e.upload_contacts(r, c, v)
        e.set_params(inp["param_simu"])
        e.upload_frags({k: np.asarray(x) for k, x in inp["S_o_A_frags"].items()})
        e.relabel_contigs()
        want = e.eval_full()
    finally:
        e.close()
    got, old = full_logl(out), full_logl(inp)
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert abs(old - want) > 1e-6 * abs(want)


def test_inactive_fragments_only_exist_with_repeats():
    """Why no GPU case above holds an inactive fragment: the engine accepts activ = 0 only for copies of repeated bins
    (graal_upload_frags), and the simulator refuses repeated bins (test_repeats_unsupported).  The kernel still gives an inactive
    fragment's sub-fragments no contacts (label -1); the numpy reference's handling is tested in tests/test_simulate_cpu.py."""
    P, par = _case("sub1")
    s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
    s["activ"][5] = 0
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.set_params(par)
        with pytest.raises(GraalError, match="activ"):
            e.upload_frags(s)
    finally:
        e.close()
