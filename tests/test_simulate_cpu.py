"""The simulator's test-side reference (tests/sim_reference.py) on its own, and the engine entry point without a GPU."""
import numpy as np
import pytest

from graal_amd import synth
from graal_amd.lib import Engine, GraalError
from tests import sim_reference as R


def test_philox4x32_known_answers():
    # Random123's known-answer vectors of philox4x32_10 (kat_vectors)
    assert R.philox_scalar((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert R.philox_scalar((0xffffffff,) * 4, (0xffffffff,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert R.philox_scalar((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_philox_rounds_match_numpy():
    # numpy.random.Philox is the 4x64 member of the family (same round structure, 64-bit words): the generic implementation matches
    # it on known keys and counters (numpy increments the counter before its first block)
    for key, ctr in (([5, 7], [1, 2, 3, 4]), ([2 ** 63 + 11, 3], [2 ** 64 - 1, 0, 9, 2 ** 40])):
        bg = np.random.Philox(key=np.array(key, dtype=np.uint64), counter=np.array(ctr, dtype=np.uint64))
        want = [int(x) for x in bg.random_raw(4)]
        c = list(ctr)
        c[0] = (c[0] + 1) % 2 ** 64
        if c[0] == 0:
            c[1] += 1
        assert R.philox_scalar(c, key, width=64) == want


def test_vectorised_philox_equals_scalar():
    rng = np.random.RandomState(1)
    c = rng.randint(0, 2 ** 32, size=(4, 50), dtype=np.uint64)
    seed = 0x1234_5678_9ABC_DEF0
    w = R.philox4x32(c[0], c[1], c[2], c[3], seed)
    for i in range(50):
        assert [int(x[i]) for x in w] == R.philox_scalar(c[:, i], (seed & R.M32, seed >> 32))


def _small(n_bins=40, n_sub=3, seed=5, accu=("random", 1, 4), v_inter=0.05, fact=300.0):
    par = synth.make_param_simu(fact=fact, v_inter=v_inter)
    P = synth.make_problem(n_bins=n_bins, nnz=200, n_sub=n_sub, seed=seed, contig_weights=(5, 3, 2), mean_len_bp=1500.0, accu=accu, param=par)
    return P, par


def test_skip_sampled_background_matches_brute_force():
    """chi^2 of the count histogram of one row's background, skip sampling + thinning + zero-truncated Poisson vs a per-pair draw."""
    P, par = _small(n_bins=300, n_sub=1, accu=("random", 1, 5), v_inter=0.4)
    rec = R.sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["S_o_A_frags"])
    nfpb = P["mean_squared_frags_per_bin"]
    S = len(rec[0])
    a = 3
    amax = int(rec[2].max())
    lmax = float(np.float32(par[7] * np.float32(np.float32(rec[2][a] * amax) / np.float32(nfpb))))
    pm = 1.0 - np.exp(-lmax)
    hist_skip = np.zeros(6)
    n_seeds = 300
    for seed in range(n_seeds):
        st = R.Stream(a, 0, 1, seed)
        j = a
        while True:
            g = -np.log(st.next()) / lmax
            if not g < float(S - j - 1):
                break
            j = j + 1 + int(np.floor(g))
            if rec[1][j] == rec[1][a] and abs(np.float32(rec[0][j] - rec[0][a])) < par[5]:
                continue
            lb = float(np.float32(par[7] * np.float32(np.float32(rec[2][a] * rec[2][j]) / np.float32(nfpb))))
            v = st.next()
            if v * pm < 1.0 - np.exp(-lb):
                hist_skip[min(R.ztp(lb, st), 5)] += 1
    rng = np.random.RandomState(0)
    hist_bf = np.zeros(6)
    for _ in range(n_seeds):
        _, c = R.brute_force_background(rec, a, a + 1, S, nfpb, par, rng)
        c = c[c > 0]
        hist_bf += np.bincount(np.minimum(c, 5), minlength=6)[:6]
    # two-sample chi^2 over the classes 1 .. 5 (pooled where sparse)
    x = np.array([hist_skip[1], hist_skip[2], hist_skip[3:].sum()])
    y = np.array([hist_bf[1], hist_bf[2], hist_bf[3:].sum()])
    chi2 = float((((x - y) ** 2) / np.maximum(x + y, 1)).sum())
    assert x.sum() > 2000 and chi2 < 16.3, (x, y, chi2)     # chi^2_3 at p = 0.001: 16.27


def test_reference_means_match_lambda():
    """Mean count per pair over seeds vs lambda, window pairs and background, n_sub 3, reversed bins, RF counts > 1."""
    P, par = _small(n_bins=24, n_sub=3, accu=("random", 1, 3), v_inter=0.3, fact=2000.0)
    s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
    s["ori"][::3] = -1
    args = (P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"], par, s)
    a, b, lam = R.expected_lambda_matrix(*args)
    S = P["init_n_sub_frags"]
    tot = np.zeros((S, S))
    n = 120
    for seed in range(n):
        r, c, v, _, _ = R.simulate(*args, seed=seed)
        assert np.all(r < c) and np.all(v > 0)
        assert np.all(np.diff(r.astype(np.int64) * S + c) > 0)
        tot[r, c] += v
    got = tot[a, b] / n
    # per pair: |mean - lambda| within 5 sigma (+ a small floor); overall: the sums within 4 sigma
    sig = np.sqrt(lam / n)
    assert np.all(np.abs(got - lam) <= 5 * sig + 0.05), np.max(np.abs(got - lam) / (sig + 1e-9))
    assert abs(got.sum() - lam.sum()) <= 4 * np.sqrt(lam.sum() / n)
    assert lam.max() > R.PTRS_MIN        # the PTRS branch is exercised


def test_inactive_fragments_get_nothing():
    P, par = _small(n_bins=30, n_sub=3)
    s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
    s["activ"][[2, 7, 19]] = 0
    r, c, v, _, _ = R.simulate(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
                               par, s, seed=3)
    dead = np.asarray(P["np_sub_frags_id"])[[2, 7, 19], :3].ravel()
    assert len(r) > 0 and not np.isin(r, dead).any() and not np.isin(c, dead).any()


def test_restricted_rows_equal_full():
    """R.simulate(rows=...) returns, for every row of a small case, exactly what the full call returns for that row -- entries in order
    and flags -- and nothing of any other row."""
    P, par = _small(n_bins=20, n_sub=3, accu=("random", 1, 4), v_inter=0.3, fact=2000.0)
    s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
    s["ori"][::3] = -1
    s["activ"][4] = 0
    args = (P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"], par, s)
    S = P["init_n_sub_frags"]

    def of_rows(full, rows):
        r, c, v, fp, fc = full
        m = np.isin(r, rows)
        return r[m], c[m], v[m], {x for x in fp if x[0] in rows}, {x for x in fc if x[0] in rows}

    def same(x, y):
        return all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(x[:3], y[:3])) and x[3] == y[3] and x[4] == y[4]

    # (TOL widened for this test alone, so that flags exist to be compared: at 1e-6 this small case has none)
    full = R.simulate(*args, seed=9)
    tol = R.TOL
    R.TOL = 1e-2
    try:
        flagged = R.simulate(*args, seed=9)
        assert len(flagged[3]) > 3 and len(flagged[4]) > 3 and len(flagged[0]) == len(full[0]) > 300
        for a in range(S):
            assert same(R.simulate(*args, seed=9, rows=[a]), of_rows(flagged, [a])), a
        some = [S - 1, 0, 17, 17, 30]
        assert same(R.simulate(*args, seed=9, rows=some), of_rows(flagged, some))
    finally:
        R.TOL = tol
    assert same(R.simulate(*args, seed=9, rows=range(S)), full)
    assert len(R.simulate(*args, seed=9, rows=[])[0]) == 0


def test_skip_near_zero_is_not_flagged():
    """A skip g > 0 cannot tip floor(g) = 0, so a row whose Lmax makes every skip tiny has no chunk flagged for it: the hubs layout's
    row 3 (Lmax = 125000, g ~ 1e-5, about 9000 skips within the old 1e-9 of 0 by chance ~ 1e-4 each)."""
    from tests.test_simulate_rows_gpu import hubs_reference
    assert not any(k[0] == 3 for k in hubs_reference()[4])


def test_hubs_layout_reaches_every_branch():
    """The conditions tests/test_simulate_rows_gpu.py relies on, on the reference alone: the row lengths its constants name, one row in
    each branch of the GPU's row sorter and at each edge between them, no flagged draw in a hub row, a background pair in the rejection
    loop of the zero-truncated Poisson, and thinning under heavy rejection."""
    from tests.test_simulate_rows_gpu import HUBS, ORDINARY, ROWS, hubs_problem, hubs_reference, reference_row
    P, par = hubs_problem()
    r, c, v, fp, fc = hubs_reference()
    assert set(np.unique(r)) <= set(ROWS)
    assert np.all(r < c) and np.all(v > 0) and np.all(np.diff(r.astype(np.int64) * P["init_n_sub_frags"] + c) > 0)
    n = {a: len(reference_row(a)[0]) for a in ROWS}
    assert {h: n[h] for h in HUBS} == {h: x[1] for h, x in HUBS.items()}
    lengths = sorted(n[h] for h in HUBS)
    assert 256 in lengths and 257 in lengths and 4096 in lengths and 4097 in lengths
    assert any(257 <= x <= 4096 and x & (x - 1) for x in lengths)          # bitonic padding
    assert any(4097 <= x <= 8192 for x in lengths) and any(x > 8192 for x in lengths)
    # exact equality on the GPU needs hub rows without a flagged draw: if this fails, choose another hub id or seed
    assert not [p for p in fp if p[0] in HUBS] and not [k for k in fc if k[0] in HUBS], (fp, fc)
    # background pairs (not in the cis window) with lambda >= 10 and a count: sim_ztp's rejection loop around sim_poisson
    centre, label, acc, lbp = R.sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["S_o_A_frags"])
    window = (label[r] == label[c]) & (np.abs(centre[c] - centre[r]).astype(np.float32) < par[5])
    lam_b = float(par[7]) * acc[r] * acc[c]
    assert (~window & (lam_b >= R.PTRS_MIN)).sum() >= 10 and lam_b[~window].max() > 1e5
    # ordinary rows: RF count 1, Lmax = v_inter * 25000 = 5 against lambda_b = 2e-4 for all but the hub columns
    assert all(acc[a] == 1 for a in ORDINARY) and np.median(acc) == 1
    assert acc.max() / np.median(acc) >= 1000                              # = Lmax / lambda_b: v_inter and the row's RF count cancel
    assert sum(n[a] > 0 for a in ORDINARY) >= 8
    # ... and they accept: a background entry in an ordinary row, in a column of RF count 1 (acceptance 4e-5 per candidate) or not
    m = np.isin(r, ORDINARY) & ~window
    assert m.sum() >= 4, m.sum()


def _failed_handle():
    """A handle whose graal_create failed for lack of a GPU (it is returned anyway, so that graal_last_error works)."""
    import ctypes
    from graal_amd import build as gbuild
    from graal_amd import lib
    gbuild.build_hip()                           # (the library cross-compiles without a GPU)
    L = lib.load()
    h = ctypes.c_void_p()
    rc = L.graal_create(0, ctypes.byref(h))
    if rc == 0:
        L.graal_destroy(h)
        pytest.skip("a GPU is present: tests/test_simulate_gpu.py covers the engine")
    return L, h


def test_simulate_entry_points_refuse_without_gpu():
    """graal_simulate_contacts / graal_simulate_fetch on a handle without a device: an error code and text, nothing drawn, no fallback;
    Engine.simulate_contacts on such a handle raises GraalError."""
    import ctypes
    from graal_amd import lib
    L, h = _failed_handle()
    try:
        nnz = ctypes.c_int64(-7)
        rc = L.graal_simulate_contacts(h, ctypes.c_uint64(1), ctypes.byref(nnz))
        assert rc != 0 and nnz.value == 0
        assert L.graal_last_error(h).decode()
        buf = np.zeros(4, np.int32)
        p = buf.ctypes.data_as(lib._i32p)
        assert L.graal_simulate_fetch(h, p, p, p, 4) != 0
        e = Engine.__new__(Engine)                   # an Engine around the failed handle: the call must raise, not fall back
        e._L, e._h = L, h
        with pytest.raises(GraalError, match="graal_simulate_contacts"):
            e.simulate_contacts(1)
        e._h = None
    finally:
        L.graal_destroy(h)


def test_engine_without_gpu_raises():
    _failed_handle()                             # (skips with a GPU)
    with pytest.raises(GraalError):
        Engine(0)


def _reference_simulator(monkeypatch):
    """simulate_problem with the GPU call replaced by the numpy reference (the same list, by the equality tests on the GPU)."""
    from graal_amd import simulate as gsim

    def fake(problem, seed, param=None, device=0):
        par = np.asarray(problem["param_simu"] if param is None else param, dtype=np.float32)
        r, c, v, _, _ = R.simulate(problem["np_sub_frags_id"], problem["np_sub_frags_len_bp"], problem["np_sub_frags_accu"],
                                   problem["mean_squared_frags_per_bin"], par, problem["S_o_A_frags"], seed)
        return r, c, v
    monkeypatch.setattr(gsim, "simulate_contacts", fake)
    return gsim


def pyramid_problem(folder, level=1):
    from graal_amd import pyramid as pyr
    P = synth.make_problem(n_bins=240, nnz=3000, n_sub=1, seed=13, contig_weights=(5, 3, 2))
    synth.write_dataset(P, folder)
    inp = pyr.simulation_inputs(pyr.build_and_filter(folder, 2, 3), level)
    inp["param_simu"] = synth.make_param_simu(fact=300.0, v_inter=0.02)
    return inp


def test_pyramid_problem_round_trip(monkeypatch, tmp_path):
    """A pyramid.simulation_inputs dict: every contact structure the sampler reads is the simulated one afterwards."""
    from graal_amd.sampler import as_coo_upper
    gsim = _reference_simulator(monkeypatch)
    inp = pyramid_problem(str(tmp_path))
    out = gsim.simulate_problem(inp, 4)
    r, c, v = gsim.simulate_contacts(inp, 4)
    assert len(v) > 100 and not np.array_equal(np.asarray(inp["hic_matrix"][2])[:len(v)], v)
    sub = as_coo_upper(out["hic_matrix"])                        # the likelihood's observations, as the sampler takes them
    assert all(np.array_equal(np.asarray(x, np.int64), np.asarray(y, np.int64)) for x, y in zip(sub, (r, c, v)))
    # the bin-level list of the neighbour proposal: the simulated counts summed per pair of different bins
    ids = np.asarray(inp["np_sub_frags_id"])
    bin_of = np.zeros(int(inp["init_n_sub_frags"]), np.int64)
    for k in range(3):
        m = ids[:, 3] > k
        bin_of[ids[m, k]] = np.nonzero(m)[0]
    nb = len(ids)
    want = {}
    for a, b, x in zip(bin_of[r], bin_of[c], v):
        if a != b:
            key = (min(a, b), max(a, b))
            want[key] = want.get(key, 0) + int(x)
    br, bc, bv = as_coo_upper(out["hic_matrix_sub_sampled"])
    assert {(int(a), int(b)): int(x) for a, b, x in zip(br, bc, bv)} == want and nb > 0
    # mean_value_trans by the reference loader's convention (pyramid.py): stored trans sum / float32(ordered trans pair count)
    id_c = np.asarray(inp["S_o_A_frags"]["id_c"])[bin_of]
    sizes = np.unique(id_c, return_counts=True)[1].astype(np.int64)
    n_tot = int((sizes * len(id_c)).sum() - (sizes * sizes).sum())
    assert out["mean_value_trans"] == np.float64(int(v[id_c[r] != id_c[c]].sum())) / np.float64(np.float32(n_tot))
    assert out["S_o_A_frags"] is inp["S_o_A_frags"]            # the layout is G0


def test_synth_problem_with_dense_round_trip(monkeypatch):
    gsim = _reference_simulator(monkeypatch)
    P, par = _small(n_bins=30, n_sub=3)
    P = synth.with_dense(P)
    out = gsim.simulate_problem(P, 2)
    r, c, v = gsim.simulate_contacts(P, 2)
    assert np.array_equal(out["coo_val"], v)
    assert np.array_equal(out["hic_matrix"], synth.dense_from_coo(r, c, v, P["init_n_sub_frags"]))
    assert np.array_equal(out["hic_matrix_sub_sampled"], synth.dense_from_coo(out["bin_coo_row"], out["bin_coo_col"], out["bin_coo_val"], P["n_frags"]))


def test_repeated_bins_refused(monkeypatch):
    gsim = _reference_simulator(monkeypatch)
    P, par = _small(n_bins=30, n_sub=1)
    with pytest.raises(ValueError, match="repeated"):
        gsim.simulate_problem(synth.add_repeats(P, [2], 1), 1)
