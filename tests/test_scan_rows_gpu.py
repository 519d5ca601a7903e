"""GPU: the two producers of a step's contacts -- the streaming pass over the whole contact list (k_scan) and the pass over the
affected rows through the row index (k_scan_rows) -- must be indistinguishable downstream.

For every case the SAME evaluations run on ONE engine with graal_set_scan_path(1) (streaming) and (2) (indexed):

* the float64 deltas are np.array_equal (they are functions of int64 sums: no tolerance);
* graal_last_counters' [1] (doubly-affected contacts) and [2] (queued contacts) are equal, and [2] equals a numpy count made
  from the COO arrays -- contacts whose row and col ids both belong to the affected contigs --, an oracle that depends on
  neither kernel;
* the indexed run's `indexed_passes` (graal_run_counters) grows by the number of evaluations, the streaming run's by zero;
* every case's numpy count is >= 1 (neighbours are drawn from the contact map), so no case passes on an empty queue.

Two and three ranks on shards of the list -- every rank indexes its own shard and chooses for itself -- are in
tests/test_multirank_gpu.py; the kernel's own branches at mid-size shapes in tests/test_scan_rows_midsize_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from graal_amd import em, synth
from tests import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM, INDEXED = 1, 2


def make(n_sub, seed, n_bins, nnz, accu=None):
    accu = (1 if n_sub == 1 else 9) if accu is None else accu
    par = synth.make_param_simu(fact=300.0, v_inter=0.03)
    return synth.make_problem(n_bins=n_bins, nnz=nnz, n_sub=n_sub, seed=seed, contig_weights=(5, 3, 2), mean_len_bp=1500.0,
                              accu=accu, param=par)


def engine_for(P, state, coo=None):
    from graal_amd.lib import Engine
    e = Engine(0)
    e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                      P["mean_squared_frags_per_bin"])
    row, col, val = coo if coo is not None else (P["coo_row"], P["coo_col"], P["coo_val"])
    e.upload_contacts(row, col, val)
    e.set_params(P["param_simu"])
    e.upload_frags(state)
    return e


def layout(P, rng, n_contigs, p_circ=0.2):
    """A random valid layout of P's fragments with n_contigs contigs (tests/util.random_layout with P's lengths)."""
    s = util.random_layout(rng, P["n_frags"], n_contigs=n_contigs, p_circ=p_circ)
    s["len_bp"][:] = P["S_o_A_frags"]["len_bp"]
    for lab in np.unique(s["id_c"]):
        m = np.nonzero(s["id_c"] == lab)[0]
        order = m[np.argsort(s["pos"][m])]
        s["start_bp"][order] = np.cumsum(s["len_bp"][order]) - s["len_bp"][order]
        s["l_cont_bp"][order] = s["len_bp"][order].sum()
    return s


def layout_of_groups(P, rng, groups, rest_max=12, p_rev=0.4):
    """A valid layout of P's fragments in which every array of `groups` is one linear contig of exactly those fragments, in that order;
    the fragments left over go, shuffled, into contigs of 1 .. rest_max fragments."""
    from oracle import oracle as O
    n = P["n_frags"]
    groups = [np.asarray(g, np.int64) for g in groups]
    used = np.concatenate(groups) if groups else np.zeros(0, np.int64)
    assert len(np.unique(used)) == len(used) and (len(used) == 0 or (used.min() >= 0 and used.max() < n))
    rest = rng.permutation(np.setdiff1d(np.arange(n), used))
    while len(rest):
        k = int(rng.randint(1, rest_max + 1))
        groups.append(rest[:k])
        rest = rest[k:]
    s = O.new_state(n)
    s["len_bp"][:] = P["S_o_A_frags"]["len_bp"]
    s["ori"][:] = np.where(rng.random_sample(n) < p_rev, -1, 1)
    s["id"][:] = np.arange(n)
    s["id_d"][:] = np.arange(n)
    for lab, g in enumerate(groups):
        lens = s["len_bp"][g].astype(np.int64)
        s["pos"][g] = np.arange(len(g))
        s["id_c"][g] = lab
        s["start_bp"][g] = np.cumsum(lens) - lens
        s["l_cont"][g] = len(g)
        s["l_cont_bp"][g] = lens.sum()
        s["prev"][g] = np.concatenate([[-1], g[:-1]])
        s["next"][g] = np.concatenate([g[1:], [-1]])
    return s


def map_neighbours(P, fA, K, rng):
    """K distinct bins that share a contact with bin fA, drawn from the bin-level contact map (so that the contact between fA
    and each of them is doubly affected: the step's queue is never empty)."""
    bi, bj = P["bin_coo_row"], P["bin_coo_col"]
    nb = np.unique(np.concatenate([bj[bi == fA], bi[bj == fA]]))
    nb = nb[nb != fA]
    assert len(nb) >= 1, "bin %d has no contact: choose another seed" % fA
    if len(nb) > K:
        nb = rng.choice(nb, K, replace=False)
    return np.sort(nb).astype(np.int32)


def numpy_count(P, state, fA, fBs, row=None, col=None):
    """Contacts whose row and col ids both belong to the contigs of fA and of the neighbours: from the COO arrays alone."""
    row = P["coo_row"] if row is None else row
    col = P["coo_col"] if col is None else col
    contigs = np.unique(state["id_c"][np.asarray([fA] + [int(f) for f in fBs])])
    bins = np.isin(state["id_c"], contigs)
    sub = bins[P["bin_of_sub"]]
    return int(np.count_nonzero(sub[row] & sub[col]))


def both_paths(e, P, state, evals, max_id, row=None, col=None):
    """Run `evals` = [(fA, fBs)] with each producer; compare deltas and counters, check both against the numpy count."""
    got = {}
    for path in (STREAM, INDEXED):
        e.set_scan_path(path)
        before = e.run_counters()
        out = []
        for fA, fBs in evals:
            d = e.eval_candidates(int(fA), np.asarray(fBs, np.int32), max_id)
            c = e.last_counters()
            out.append((d, int(c[1]), int(c[2])))
        after = e.run_counters()
        assert after["fallbacks"] == before["fallbacks"]
        grown = after["indexed_passes"] - before["indexed_passes"]
        assert grown == (len(evals) if path == INDEXED else 0), (path, grown)
        got[path] = out
    e.set_scan_path(0)
    for (fA, fBs), a, b in zip(evals, got[STREAM], got[INDEXED]):
        want = numpy_count(P, state, fA, fBs, row, col)
        assert want >= 1, (fA, fBs)
        assert a[1] == b[1] and a[2] == b[2], (fA, fBs, a[1:], b[1:])
        assert b[2] == want and b[1] == want, (fA, fBs, b[1:], want)
        assert np.array_equal(a[0], b[0]), (fA, fBs)
        assert np.isfinite(a[0]).all()
    return got


def set_arithmetic(e, which):
    e.set_mode(ref_trans_accu=which == "strict", strict=which == "strict")


@pytest.mark.parametrize("which", ["exact", "strict"])
def test_short_contigs_one_sub_fragment_per_bin(which):
    P = make(1, 71, 400, 30000)
    rng = np.random.RandomState(71)
    s = layout(P, rng, 150)
    e = engine_for(P, s)
    set_arithmetic(e, which)
    max_id = e.relabel_contigs()
    evals = [(int(f), map_neighbours(P, int(f), 5, rng)) for f in rng.choice(P["n_frags"], 8, replace=False)]
    both_paths(e, P, s, evals, max_id)
    e.close()


@pytest.mark.parametrize("which", ["exact", "strict"])
def test_three_sub_fragments_per_bin_with_mixed_rf_counts(which):
    P = make(3, 72, 240, 40000, accu=("random", 3, 12))
    rng = np.random.RandomState(72)
    s = layout(P, rng, 90)
    e = engine_for(P, s)
    set_arithmetic(e, which)
    max_id = e.relabel_contigs()
    evals = [(int(f), map_neighbours(P, int(f), 5, rng)) for f in rng.choice(P["n_frags"], 8, replace=False)]
    both_paths(e, P, s, evals, max_id)
    e.close()


@pytest.mark.parametrize("n_sub,which", [(1, "exact"), (1, "strict"), (3, "strict")])
def test_contig_longer_than_the_mates_rows(n_sub, which):
    """fA (or a neighbour) in a contig of more than 8 fragments: the prologue marks it from the position index."""
    P = make(n_sub, 73, 300, 30000)
    rng = np.random.RandomState(73)
    s = layout(P, rng, 20)   # mean 15 fragments per contig
    long_frags = np.nonzero(s["l_cont"] > 8)[0]
    short_frags = np.nonzero(s["l_cont"] <= 8)[0]
    assert len(long_frags) >= 8
    e = engine_for(P, s)
    set_arithmetic(e, which)
    max_id = e.relabel_contigs()
    evals = [(int(f), map_neighbours(P, int(f), 5, rng)) for f in rng.choice(long_frags, 6, replace=False)]
    if len(short_frags):   # a short fA whose neighbours are (mostly) in long contigs
        f = int(short_frags[0])
        evals.append((f, map_neighbours(P, f, 5, rng)))
    both_paths(e, P, s, evals, max_id)
    e.close()


def test_neighbour_lists_with_shared_contigs_duplicates_and_fa_itself():
    P = make(1, 74, 300, 30000)
    rng = np.random.RandomState(74)
    s = layout(P, rng, 60, p_circ=0.0)
    e = engine_for(P, s)
    max_id = e.relabel_contigs()
    evals = []
    for fA in rng.choice(np.nonzero((s["l_cont"] >= 3) & (s["l_cont"] <= 8))[0], 3, replace=False):
        fA = int(fA)
        nb = map_neighbours(P, fA, 3, rng)
        mate = int(np.nonzero((s["id_c"] == s["id_c"][fA]) & (np.arange(P["n_frags"]) != fA))[0][0])
        evals.append((fA, np.sort(np.append(nb, mate)).astype(np.int32)))          # fA in the same contig as a neighbour
        evals.append((fA, np.sort(np.append(nb, nb[0])).astype(np.int32)))         # a neighbour listed twice
        evals.append((fA, np.sort(np.append(nb, fA)).astype(np.int32)))            # fA = a neighbour
    both_paths(e, P, s, evals, max_id)
    e.close()


def test_a_row_without_contacts_and_the_last_id():
    """The last id of the list is never a row (row < col), and a bin that only ever appears as a col has an empty row: the
    indexed pass finds their contacts through the OTHER end's row."""
    P = make(1, 75, 300, 30000)
    rng = np.random.RandomState(75)
    s = layout(P, rng, 110)
    S = P["init_n_sub_frags"]
    last = S - 1
    assert not np.any(P["coo_row"] == last) and np.any(P["coo_col"] == last)
    empty = np.setdiff1d(np.unique(P["coo_col"]), np.unique(P["coo_row"]))
    assert last in empty
    e = engine_for(P, s)
    max_id = e.relabel_contigs()
    evals = [(int(f), map_neighbours(P, int(f), 5, rng)) for f in empty[-3:]]
    f = int(P["coo_row"][np.nonzero(P["coo_col"] == last)[0][0]])
    evals.append((f, np.sort(np.append(map_neighbours(P, f, 3, rng), last)).astype(np.int32)))   # ... and as a neighbour
    both_paths(e, P, s, evals, max_id)
    e.close()


@pytest.mark.parametrize("K", [1, 10])
def test_one_and_ten_neighbours(K):
    P = make(1, 76, 400, 40000)
    rng = np.random.RandomState(76)
    s = layout(P, rng, 140)
    e = engine_for(P, s)
    set_arithmetic(e, "strict")
    max_id = e.relabel_contigs()
    evals = []
    for f in rng.choice(P["n_frags"], 6, replace=False):
        nb = map_neighbours(P, int(f), K, rng)
        if len(nb) == K:
            evals.append((int(f), nb))
    assert len(evals) >= 3
    both_paths(e, P, s, evals, max_id)
    e.close()


def test_unsorted_list_has_no_index_and_streams():
    P = make(1, 77, 300, 30000)
    rng = np.random.RandomState(77)
    s = layout(P, rng, 110)
    perm = rng.permutation(len(P["coo_row"]))
    row, col, val = P["coo_row"][perm], P["coo_col"][perm], P["coo_val"][perm]
    from graal_amd.lib import GraalError
    e_sorted = engine_for(P, s)
    e_uns = engine_for(P, s, coo=(row, col, val))
    with pytest.raises(GraalError, match="row index|sorted"):
        e_uns.set_scan_path(INDEXED)
    m1, m2 = e_sorted.relabel_contigs(), e_uns.relabel_contigs()
    assert m1 == m2
    e_sorted.set_scan_path(INDEXED)
    for f in rng.choice(P["n_frags"], 5, replace=False):
        nb = map_neighbours(P, int(f), 5, rng)
        want = numpy_count(P, s, int(f), nb)
        assert want >= 1
        a = e_uns.eval_candidates(int(f), nb, m2)       # auto: no index, streams
        ca = e_uns.last_counters()
        b = e_sorted.eval_candidates(int(f), nb, m1)
        cb = e_sorted.last_counters()
        assert np.array_equal(a, b)
        assert int(ca[2]) == int(cb[2]) == want
    assert e_uns.run_counters()["indexed_passes"] == 0
    assert e_sorted.run_counters()["indexed_passes"] == 5
    e_sorted.close()
    e_uns.close()


def sampler_problem():
    par = synth.make_param_simu(fact=200.0, v_inter=0.02)
    return synth.make_problem(n_bins=150, nnz=6000, n_sub=1, seed=78, contig_weights=(5, 4, 3), mean_len_bp=2000.0, accu=1, param=par,
                              grid_bp=2000)


def switch_problem():
    """3,000 bins, 1,000,000 contacts, longest row 661: with K = 4 the engine's own choice is the indexed pass while the bound on the longest
    contig is at most 18 fragments and the streaming pass from 19 on (5 x 19 x 661 x 16 > 1,000,000) -- a run from the exploded layout starts
    indexed and changes producer once a contig of 9 fragments exists (the bound between relabels is 2 x 9 + 2).
    tests/test_scan_rows_reference_cpu.py checks these figures."""
    par = synth.make_param_simu(fact=200.0, v_inter=0.02)
    return synth.make_problem(n_bins=3000, nnz=1_000_000, n_sub=1, seed=88, contig_weights=(5, 4, 3), mean_len_bp=2000.0, accu=1, param=par,
                              grid_bp=2000)


def sampler_run(path, cycles, problem=sampler_problem):
    """cycles x n_bins graal_step steps from the exploded layout with one producer (0: the engine's own choice); what a run leaves behind."""
    from tests.test_sampler_gpu import make_gpu_sampler
    P = problem()
    rng = np.random.RandomState(78)
    g = make_gpu_sampler(P, rng)
    g.engine.set_scan_path(path)
    t = em.run_em(g, cycles, 4, rng=rng)
    st = rng.get_state(legacy=False)["state"]
    rc = g.engine.run_counters()
    out = dict(mutations=np.asarray(t.mutations()).tolist(), likelihood=[float(v) for v in t.likelihood], n_contigs=[int(v) for v in t.n_contigs],
               pos=int(st["pos"]), key=[int(v) for v in st["key"]], used_c=bool(g._c_step), evaluations=rc["evaluations"],
               indexed=rc["indexed_passes"], fallbacks=rc["fallbacks"])
    g.free_gpu()
    return out


def _child_run():
    print("RESULT " + json.dumps(sampler_run(INDEXED, 1)))


def _child_switch_run():
    print("RESULT " + json.dumps(sampler_run(0, 2, switch_problem)))


def same_run(a, b):
    assert a["mutations"] == b["mutations"]
    assert a["likelihood"] == b["likelihood"] and a["n_contigs"] == b["n_contigs"]
    assert a["pos"] == b["pos"] and a["key"] == b["key"]


def test_600_steps_from_the_exploded_layout():
    a, b = sampler_run(STREAM, 4), sampler_run(INDEXED, 4)
    assert a["used_c"] and b["used_c"]
    assert len(a["mutations"]) >= 1 and a["n_contigs"][-1] < 0.7 * 150     # the runs did something
    same_run(a, b)
    # (600 steps; a step whose fragment has no neighbour in the contact map evaluates nothing)
    assert a["indexed"] == 0 and a["evaluations"] >= 450
    assert b["indexed"] == b["evaluations"] == a["evaluations"]
    assert a["fallbacks"] == 0 and b["fallbacks"] == 0


def test_forced_time_out_with_the_indexed_producer():
    """GRAAL_TM_SPIN_TICKS=1 (read when the engine is created: a child process): k_tm gives up waiting for the producer's
    announcement at once, the step is repeated behind events -- with the producer it had -- and the run equals the streaming one."""
    env = dict(os.environ, GRAAL_TM_SPIN_TICKS="1")
    env.pop("GRAAL_NO_TM_SPIN", None)
    env.pop("GRAAL_PY_STEP", None)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import tests.test_scan_rows_gpu as t; t._child_run()"], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    b = json.loads(line[len("RESULT "):])
    a = sampler_run(STREAM, 1)
    same_run(a, b)
    assert b["used_c"] and b["fallbacks"] >= 1, "no step was repeated: the case tests nothing"
    assert b["indexed"] == b["evaluations"]     # (a repeated step counts as an evaluation of its own, and stays indexed)


def test_the_engines_own_choice_changes_producer_within_a_run(monkeypatch):
    """Two cycles (6,000 steps) from the exploded layout of switch_problem with nothing forced and the shipped ratio: the run starts with the
    indexed pass, its contigs grow -- the first contig of 9 fragments appears early in the second cycle --, and it goes over to the
    streaming pass -- relying on the bound 2 x max + 2 for the longest contig
    between relabels.  It must equal the run that streams throughout; and so must the same run in a child whose in-kernel wait for the
    producer runs out at once (GRAAL_TM_SPIN_TICKS=1), where steps are repeated behind events with the producer they had."""
    for name in ("GRAAL_SCAN_PATH", "GRAAL_SCAN_ROWS_R", "GRAAL_TM_SPIN_TICKS"):
        monkeypatch.delenv(name, raising=False)
    auto = sampler_run(0, 2, switch_problem)
    stream = sampler_run(STREAM, 2, switch_problem)
    assert auto["used_c"] and stream["used_c"] and len(auto["mutations"]) >= 1
    same_run(stream, auto)
    print("own choice: %d evaluations, %d indexed, %d fallbacks" % (auto["evaluations"], auto["indexed"], auto["fallbacks"]))
    assert stream["indexed"] == 0 and stream["evaluations"] == auto["evaluations"]
    assert auto["indexed"] >= 50 and auto["evaluations"] - auto["indexed"] >= 50, "the run did not use both producers"
    assert auto["fallbacks"] == 0
    env = {k: v for k, v in os.environ.items() if k not in ("GRAAL_NO_TM_SPIN", "GRAAL_PY_STEP")}
    env["GRAAL_TM_SPIN_TICKS"] = "1"
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "import tests.test_scan_rows_gpu as t; t._child_switch_run()"], cwd=ROOT,
                       env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    b = json.loads(line[len("RESULT "):])
    same_run(stream, b)
    print("own choice, waits run out: %d evaluations, %d indexed, %d fallbacks" % (b["evaluations"], b["indexed"], b["fallbacks"]))
    assert b["used_c"] and b["fallbacks"] >= 1, "no step was repeated: the case tests nothing"
    assert b["indexed"] >= 1 and b["evaluations"] - b["indexed"] >= 1


def test_c5_size_exploded_layout_auto_takes_the_index():
    """The benchmark's map (50,000 fragments, 20,000,000 contacts) in its exploded layout: both producers agree, and the engine's own
    choice (auto, no event pairs) is the indexed pass."""
    import bench
    P = synth.make_problem(n_bins=50000, nnz=20_000_000, n_sub=1, seed=20141217)
    P["S_o_A_frags"] = bench.exploded_layout(P)
    rng = np.random.RandomState(79)
    smp = bench.build_sampler(P, rng, None, 0)
    smp.init_likelihood()
    e = smp.engine
    e.set_timing(0)
    max_id = smp.modify_gl_cuda_buffer(0)
    smp.gpu_vect_frags.copy_from_gpu()
    state = {"id_c": np.copy(smp.gpu_vect_frags.id_c)}
    evals = []
    for f in rng.randint(0, 50000, size=6):
        nb = smp.return_neighbours(int(f), 5)
        nb.sort()
        evals.append((int(f), np.asarray(nb, np.int32)))
    got = both_paths(e, P, state, evals, max_id)
    before = e.run_counters()["indexed_passes"]
    for (fA, fBs), ref in zip(evals, got[STREAM]):
        assert np.array_equal(e.eval_candidates(fA, fBs, max_id), ref[0])
    assert e.run_counters()["indexed_passes"] - before == len(evals)
    e.set_timing(1)      # an evaluation that carries an event pair streams
    before = e.run_counters()["indexed_passes"]
    assert np.array_equal(e.eval_candidates(evals[0][0], evals[0][1], max_id), got[STREAM][0][0])
    assert e.run_counters()["indexed_passes"] == before
    e.set_timing(0)
    smp.free_gpu()
