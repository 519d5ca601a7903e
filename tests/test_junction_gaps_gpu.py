"""graal_junction_gaps on the GPU: the data's own scores word for word those of graal_junction_scores, every cell of the profile equal to
the numpy restatement (tests/junction_gap_reference.py) within the project's bound, zeros at gap 0, minus the junction score at gaps
>= d_max, the same with and without the trans-branch indexing, best / q_best / lo / hi exactly those of the returned matrix,
deterministic and independent of the grid a value stands in and of the batching, refused where graal_junction_scores is, free of side
effects on a run, the table the CLI writes, and sound on simulated data with planted gaps."""
import ctypes
import functools
import mmap
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from graal_amd import em, junctions, synth
from graal_amd.lib import Engine, GraalError, JUNCTION_CIRCULAR, JUNCTION_VALID
from tests import junction_gap_reference as GR
from tests import junction_reference as JR
from tests.test_junctions_gpu import _layout, engine_for

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sub3", "sub1", "circ")
CASES = [pytest.param(n, q, id="%s-%d" % (n, q)) for n in NAMES for q in (False, True)]
SUB = (0, 5, 9)                                              # the call of three values: these of the grid of 11
FOLD_KEYS = ("best", "q_best", "lo", "hi")


def tol(A):
    return 1e-9 * np.asarray(A, np.float64) + 1           # tests/test_layout_scores_midsize_gpu.py's bound, in Q


@functools.lru_cache(maxsize=None)
def gpu(name, quirk):
    """One engine per case and mode: graal_junction_scores, then the profile on the grid of 11 twice, without the matrix, at drop 0, at
    a drop taken from the matrix and at one less, on 3 of the 11 values and on 19 that hold the 11."""
    P = JR.case(name)
    grid = GR.small_grid(P)
    e = engine_for(P, quirk=quirk)
    try:
        out = {"scores": e.junction_scores_q()}
        out["full"] = e.junction_gaps_q(grid, GR.DROP_Q, profile=True)
        out["again"] = e.junction_gaps_q(grid, GR.DROP_Q, profile=True)
        out["plain"] = e.junction_gaps_q(grid, GR.DROP_Q)
        out["zero"] = e.junction_gaps_q(grid, 0, profile=True)
        g = out["full"]
        ok = np.nonzero(g["status"] == JUNCTION_VALID)[0]
        f = ok[len(ok) // 2]
        col = np.unique(g["q_gap"][:, f])
        out["drop"] = int(col[-1] - col[-2])                 # the step from the largest value of f's profile to the next one
        out["at_drop"] = e.junction_gaps_q(grid, out["drop"], profile=True)
        out["below_drop"] = e.junction_gaps_q(grid, out["drop"] - 1, profile=True)
        out["three"] = e.junction_gaps_q(grid[list(SUB)], GR.DROP_Q, profile=True)
        out["wide"] = e.junction_gaps_q(GR.wide_grid(P), GR.DROP_Q, profile=True)
        out["scores_after"] = e.junction_scores_q()
    finally:
        e.close()
    return out


@pytest.mark.parametrize("name,quirk", CASES)
def test_data_scores_are_junction_scores(name, quirk):
    g = gpu(name, quirk)
    q, st = g["scores"]
    for k in ("full", "plain", "zero", "at_drop", "three", "wide"):
        assert np.array_equal(g[k]["q"], q) and np.array_equal(g[k]["status"], st), k
    assert np.array_equal(g["scores_after"][0], q) and np.array_equal(g["scores_after"][1], st)
    assert (st == JUNCTION_VALID).sum() >= 10
    s = JR.case(name)["S_o_A_frags"]
    ring = np.asarray(s["circ"]) == 1
    assert ring.any() == (name == "circ") and (st[ring] == JUNCTION_CIRCULAR).all()
    for k in FOLD_KEYS:
        assert not g["full"][k][st != JUNCTION_VALID].any(), k
    assert not g["full"]["q_gap"][:, st != JUNCTION_VALID].any()


@pytest.mark.parametrize("name,quirk", CASES)
def test_profile_equals_restatement(name, quirk):
    g = gpu(name, quirk)["full"]
    P, grid, G, st, A = GR.small(name)
    assert np.array_equal(g["status"], st) and g["q_gap"].shape == G.shape == (11, len(st))
    ok = st == GR.VALID
    excess = np.abs(g["q_gap"] - G)[:, ok] / tol(A[:, ok])
    print("%s quirk %d: %d cells, largest |q_gap - G| / tolerance %.3e" % (name, quirk, excess.size, float(excess.max())))
    assert (excess <= 1).all(), int((excess > 1).sum())
    assert not g["q_gap"][0].any()                           # gap 0: every term is exactly 0
    # a gap as wide as the window is a cut in the plain indexing: minus the junction score without the mode flag
    d_max = np.float32(P["param_simu"][5])
    wide = np.nonzero(grid >= d_max)[0]
    J = gpu(name, False)["scores"][0]
    assert len(wide) == 2
    for r in wide:
        diff = np.abs(g["q_gap"][r] + J)[ok]
        print("%s quirk %d: gap %.1f kb, largest |q_gap + q_out| %d (in Q)" % (name, quirk, grid[r], int(diff.max())))
        assert (diff <= tol(A[r][ok])).all()
    inner = g["q_gap"][1:wide[0]][:, ok]
    assert (inner != 0).all() and (np.diff(g["q_gap"][:wide[0] + 1][:, ok], axis=0) != 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_mode_flag_changes_nothing(name):
    a, b = gpu(name, False), gpu(name, True)
    for call in ("full", "zero", "three", "wide"):
        for k in FOLD_KEYS + ("q_gap",):
            assert np.array_equal(a[call][k], b[call][k]), (call, k)
    if name == "sub3":
        assert not np.array_equal(a["scores"][0], b["scores"][0])   # (the junction scores themselves do move)


@pytest.mark.parametrize("name,quirk", CASES)
def test_fold_is_that_of_the_matrix(name, quirk):
    G = gpu(name, quirk)
    drop = G["drop"]
    assert drop > 0
    for call, d in (("full", GR.DROP_Q), ("zero", 0), ("at_drop", drop), ("below_drop", drop - 1), ("three", GR.DROP_Q), ("wide", GR.DROP_Q)):
        g = G[call]
        want = GR.fold(g["q_gap"], g["status"], d)
        for k, w in zip(FOLD_KEYS, want):
            assert np.array_equal(g[k], w) and g[k].dtype == w.dtype, (call, k)
    ok = G["full"]["status"] == JUNCTION_VALID
    z = G["zero"]
    assert np.array_equal(z["lo"], z["best"]) and (z["hi"] >= z["best"]).all()
    assert (G["full"]["lo"][ok] < G["full"]["hi"][ok]).any() and (G["full"]["best"][ok] > 0).any()
    # the drop taken from the matrix is met with equality: it moves lo or hi, one less does not
    moved = (G["at_drop"]["lo"] != G["below_drop"]["lo"]) | (G["at_drop"]["hi"] != G["below_drop"]["hi"])
    assert moved.any() and np.array_equal(G["at_drop"]["best"], G["below_drop"]["best"])


@pytest.mark.parametrize("name,quirk", CASES)
def test_deterministic_whatever_the_grid_and_the_batching(name, quirk):
    G = gpu(name, quirk)
    full = G["full"]
    for k in full:
        assert np.array_equal(full[k], G["again"][k]), k
    for k in ("q", "status") + FOLD_KEYS:
        assert np.array_equal(full[k], G["plain"][k]), k
    assert "q_gap" not in G["plain"]
    for call in ("zero", "at_drop", "below_drop"):
        assert np.array_equal(G[call]["q_gap"], full["q_gap"]), call
    # a row depends on its own gap value alone: three of the 11, and 19 that hold the 11 -- more than two launches of the mass kernel
    src = open(os.path.join(ROOT, "graal_amd", "csrc", "junction_gaps.h")).read()
    gb = int(re.search(r"constexpr int JG_GB = (\d+);", src).group(1))
    assert 19 > 2 * gb and 11 > gb > 3
    assert np.array_equal(G["three"]["q_gap"], full["q_gap"][list(SUB)])
    P = JR.case(name)
    grid, wide = GR.small_grid(P), GR.wide_grid(P)
    at = np.searchsorted(wide, grid)
    assert len(wide) == 19 and np.array_equal(wide[at], grid)
    assert np.array_equal(G["wide"]["q_gap"][at], full["q_gap"])
    ok = full["status"] == JUNCTION_VALID
    rest = np.setdiff1d(np.arange(19), at)
    assert (G["wide"]["q_gap"][rest][:, ok] != 0).all()


def test_float_columns():
    name = "sub3"
    P = JR.case(name)
    grid = GR.small_grid(P)
    G = gpu(name, False)["full"]
    e = engine_for(P)
    try:
        f = e.junction_gaps(grid, profile=True)
        t = junctions.gap_table(e, grid)
        d = junctions.gap_table(e, points=9)
        J, _ = e.junction_scores()
        soa = e.download_frags()
    finally:
        e.close()
    ok = G["status"] == JUNCTION_VALID
    Qs = float(1 << 30)
    g64 = grid.astype(np.float64)
    assert np.array_equal(f["status"], G["status"]) and all(np.isnan(f[k][~ok]).all() for k in ("J", "gap_kb", "gap_score", "gap_lo_kb", "gap_hi_kb"))
    assert np.isnan(f["profile"][:, ~ok]).all() and np.array_equal(f["profile"][:, ok], G["q_gap"][:, ok] / Qs)
    assert np.array_equal(f["gap_kb"][ok], g64[G["best"][ok]]) and np.array_equal(f["gap_score"][ok], G["q_best"][ok] / Qs)
    assert np.array_equal(f["gap_lo_kb"][ok], g64[G["lo"][ok]]) and np.array_equal(f["gap_hi_kb"][ok], g64[G["hi"][ok]])
    assert np.array_equal(f["J"][ok], J[ok]) and all(np.array_equal(f[k], G[k]) for k in ("best", "lo", "hi"))
    assert tuple(t) == junctions.GAP_COLUMNS and len(t["gap_kb"]) == ok.sum()
    lf = t["left_frag"]
    assert np.array_equal(t["gap_kb"], f["gap_kb"][lf]) and np.array_equal(t["score"], J[lf]) and np.array_equal(t["gap_score"], f["gap_score"][lf])
    assert np.array_equal(t["gap_open"], (G["hi"][lf] == len(grid) - 1).astype(np.float64))
    # the default grid: 0, then a quarter of the median bin length up to the model's d_max
    want = junctions.default_gap_grid(float(P["param_simu"][5]), 9, median_bin_kb=float(np.median(soa["len_bp"])) / 1000.0)
    assert set(np.unique(d["gap_kb"])) <= set(want.astype(np.float64)) and np.array_equal(d["score"], t["score"])


def test_no_side_effect_on_a_run():
    """run_em with junction_gaps_q() called at the end of every cycle and in the middle of one gives the same accepted moves and
    likelihoods (tests/test_junctions_gpu.py's pattern)."""
    from tests.test_sampler_gpu import make_gpu_sampler
    P = synth.with_dense(synth.make_problem(n_bins=70, nnz=1200, n_sub=1, seed=41, contig_weights=(5, 4, 3), mean_len_bp=2000.0,
                                            param=synth.make_param_simu(fact=200.0, v_inter=0.02), grid_bp=2000))
    n = P["n_frags"]
    grid = np.array([0.0, 0.5, 3.0, 20.0, 500.0], np.float32)
    runs = []
    for call in (False, True):
        rng = np.random.RandomState(5)
        smp = make_gpu_sampler(P, rng, reference_arithmetic="exact")
        seen, calls = [], []

        def on_step(j, i, trace, smp=smp, seen=seen, call=call, calls=calls):
            seen.append(i)
            if call and (len(seen) % n == 0 or len(seen) == n // 2):
                calls.append(smp.engine.junction_gaps_q(grid, GR.DROP_Q, profile=True))

        tr = em.run_em(smp, 3, 3, rng=rng, on_step=on_step)
        runs.append((tr.mutations(), np.array(tr.likelihood), np.array(tr.n_contigs)))
        smp.free_gpu()
        assert (len(calls) >= 3) == call
    (m0, l0, c0), (m1, l1, c1) = runs
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert np.array_equal(l0, l1)


def test_refusals():
    name = "sub1"
    P = JR.case(name)
    grid = GR.small_grid(P)
    want = gpu(name, False)["full"]
    e = engine_for(P)
    try:
        seg = mmap.mmap(-1, max(e.exchange_bytes(2), mmap.PAGESIZE))   # (rank 0 of two: a world of one has no exchange)
        e.attach_exchange(seg, 0, 2, 0)
        with pytest.raises(GraalError, match=r"one rank.*code 3\)"):
            e.junction_gaps_q(grid, 0)
        e.detach_exchange()
        bad_grids = {"descending": grid[::-1], "repeated": np.array([0.0, 1.0, 1.0], np.float32), "negative": np.array([-0.5, 1.0], np.float32),
                     "none": np.zeros(0, np.float32), "65": np.arange(65, dtype=np.float32), "nan": np.array([0.0, np.nan, 2.0], np.float32),
                     "inf": np.array([0.0, np.inf], np.float32)}
        for k, g in bad_grids.items():
            with pytest.raises(GraalError, match=r"code 1\)"):
                e.junction_gaps_q(g, 0, profile=True)
        with pytest.raises(GraalError, match=r"code 1\)"):
            e.junction_gaps_q(grid, -1)
        n = e.n
        q, qb = np.zeros(n, np.int64), np.zeros(n, np.int64)
        lo, hi = np.zeros(n, np.int32), np.zeros(n, np.int32)
        st = np.zeros(n, np.uint8)
        p64, p32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
        rc = e._L.graal_junction_gaps(e._h, grid.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(grid), 0, q.ctypes.data_as(p64),
                                      st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None, qb.ctypes.data_as(p64),
                                      lo.ctypes.data_as(p32), hi.ctypes.data_as(p32), None)
        assert rc == 1 and not q.any() and not qb.any()
        rc = e._L.graal_junction_gaps(e._h, None, len(grid), 0, q.ctypes.data_as(p64), st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                      lo.ctypes.data_as(p32), qb.ctypes.data_as(p64), lo.ctypes.data_as(p32), hi.ctypes.data_as(p32), None)
        assert rc == 1 and not q.any()
        assert len(e.junction_gaps_q(np.arange(64, dtype=np.float32), 0, profile=True)["q_gap"]) == 64   # 64 values are allowed
        got = e.junction_gaps_q(grid, GR.DROP_Q, profile=True)          # the engine works afterwards
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    finally:
        e.close()
    from tests.test_repeats_gpu import engine_with_repeats, rep_problem
    R = rep_problem(1, 7)
    e = engine_with_repeats(R, R["S_o_A_frags"])
    try:
        with pytest.raises(GraalError, match=r"code 4\)"):
            e.junction_gaps_q(np.array([0.0, 1.0], np.float32), 0)
    finally:
        e.close()


def test_simulated_genome_brackets_its_planted_gaps():
    """tests/test_junctions_gpu.py's simulated 1,000-bin genome (contacts from simulate_contacts(2024) on the true layout) with runs of
    3, 10 and 30 bins of contig 0 moved into contigs of their own and the hole closed; 41 gap values, 0 and 0.5 .. 400 kb.  First the
    restatement on these very contacts, then the engine: each planted gap lies inside [lo, hi] at drop 1.92, at least 95 % of the other
    junctions keep grid index 0 inside theirs, and the engine's profile is the restatement's within the bound.  Measured (printed
    below; one MI355X): see DESIGN.md section 8c3."""
    P, true, test, planted = GR.simulated()
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.set_params(P["param_simu"])
        e.upload_frags(true)
        r, c, v = e.simulate_contacts(2024)
        e.upload_contacts(r, c, v)
        e.upload_frags(test)
        g = e.junction_gaps_q(GR.STAT_GRID, GR.DROP_Q, profile=True)
    finally:
        e.close()
    G, st, A = GR.vectorised(dict(P, coo_row=r, coo_col=c, coo_val=v), GR.STAT_GRID, test)
    assert (st == GR.VALID).sum() == 1000 - 6 and len(GR.STAT_GRID) == 41
    for who, (prof, status) in (("restatement", (G, st)), ("engine", (g["q_gap"], g["status"]))):
        inside, share, rows = GR.check_simulated(prof, status, test, planted)
        print("%s: planted (gap, best, lo, hi kb) %s; share of the other junctions holding 0: %.4f"
              % (who, [tuple(round(x, 2) for x in row) for row in rows], share))
        assert all(inside), (who, rows)
        assert share >= 0.95, (who, share)
    assert np.array_equal(g["status"], st)
    ok = st == GR.VALID
    excess = np.abs(g["q_gap"] - G)[:, ok] / tol(A[:, ok])
    print("largest |q_gap - G| / tolerance %.3e" % float(excess.max()))
    assert (excess <= 1).all()
    for k, w in zip(FOLD_KEYS, GR.fold(g["q_gap"], g["status"], GR.DROP_Q)):
        assert np.array_equal(g[k], w), k


def test_run_writes_junction_gaps_tsv():
    """The rows are gap_table's of the layout the run ended in (its fragments, orientations and order are in the rows themselves), on a
    sampler built from the same dataset the way graal_amd.run builds its own."""
    from graal_amd import pyramid as pyr
    from graal_amd.sampler import sampler
    P = synth.make_problem(n_bins=300, nnz=3000, n_sub=1, seed=12, contig_weights=(5, 3, 2))
    par = synth.make_param_simu(fact=300.0, v_inter=0.02)
    with tempfile.TemporaryDirectory() as d:
        data, out = os.path.join(d, "data"), os.path.join(d, "out")
        synth.write_dataset(P, data)
        cmd = [sys.executable, "-m", "graal_amd.run", "--dataset", data, "--size-pyramid", "1", "--level", "0", "--cycles", "1",
               "--neighbours", "3", "--seed", "3", "--arithmetic", "exact", "--out", out, "--junctions", "--junction-gaps",
               "--junction-gaps-points", "12", "--junction-gaps-drop", "2.5", "--no-fit", "--param", *[str(float(x)) for x in par]]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = open(os.path.join(out, "junction_gaps.tsv")).read().splitlines()
        plain = open(os.path.join(out, "junctions.tsv")).read().splitlines()
        root = os.path.join(data, "pyramids", "pyramid_1_thresh_auto")
        inp = pyr.simulation_inputs(pyr.Pyramid(root, 1), 0, candidates_blacklist=[0], allow_repeats=False)
    assert lines[0].split("\t") == list(junctions.GAP_COLUMNS)
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
        t = junctions.gap_table(smp, None, 2.5, 12)
    finally:
        smp.free_gpu()
    assert np.array_equal(t["left_frag"], left) and np.array_equal(t["right_frag"], right)
    for j, c in enumerate(junctions.GAP_COLUMNS[nc - 1:]):
        got = np.array([float(x[nc - 1 + j]) for x in rows])
        assert np.array_equal(got, t[c], equal_nan=True), c
    assert set(t["gap_open"]) <= {0.0, 1.0} and (t["gap_lo_kb"] <= t["gap_kb"]).all() and (t["gap_kb"] <= t["gap_hi_kb"]).all()
