"""GPU: the sharded (multi-rank) engine path, exercised with 2-3 ranks on ONE GPU (gloo backend, all on cuda:0):
contact shards, rank-sharded mass items, one exchange of 13*K int64 sums per step -- through the pinned host segment the
ranks share (exchange="host": graal_attach_exchange / graal_eval_candidates_x) or as one all-reduce of a device buffer
(exchange="rccl": graal_eval_candidates_q + torch.distributed).  The per-candidate deltas -- and therefore the
accepted-move trace -- must be bit-identical to the single-rank run (Q30 integer sums are order independent)."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _problem(which="sub3"):
    from graal_amd import synth
    par = synth.make_param_simu(fact=200.0, v_inter=0.02)
    if which == "mid":
        # the middle of a run at one sub-fragment per bin (the C4 stand-in's regime in small): contigs of tens to hundreds of bins -- affected
        # sets beyond what k_tm prices itself: k_strict_flat, and k_gprep + k_strict2 for the larger ones -- on GENERIC bp lengths, in
        # reference arithmetic (the default)
        # (10 contigs of ~50 bins: not the late stage's direct launch of the tiled kernels -- k_tm sends every rank to k_strict_flat)
        return synth.make_problem(n_bins=500, nnz=15000, n_sub=1, seed=19, contig_weights=(1,) * 10, mean_len_bp=1500.0, accu=1, param=par)
    if which == "mid6k":
        # "mid" with a list of between one and two of the 4,096-contact blocks that graal_amd.dist.shard_take deals out: on three ranks, rank 0
        # holds one block, rank 1 the rest -- the row at the boundary is split between them -- and rank 2 nothing at all
        return synth.make_problem(n_bins=500, nnz=6000, n_sub=1, seed=19, contig_weights=(1,) * 10, mean_len_bp=1500.0, accu=1, param=par)
    if which == "rep":
        # repeated bins (allow_repeats: simulation_loader.py:182-280): their pixels are priced densely over the active copies -- the candidates'
        # part dealt to the ranks item by item, the full evaluation's part pixel by pixel (k_rep_delta, k_rep_full)
        P = synth.make_problem(n_bins=60, nnz=1500, n_sub=3, seed=23, contig_weights=(5, 4, 3), mean_len_bp=2000.0, accu=("random", 1, 9), param=par)
        return synth.add_repeats(P, (7, 21, 40), 2)
    if which == "c2":
        # the C2 stand-in (BASELINE config 2's shape: 1,086 bins x 3 sub-fragments, 120,000 contacts), generic coordinates: one cycle from the
        # exploded genome -- the table kernel, the flat kernel and the tiled kernels, the total carried with the commits' corrections
        return synth.make_problem(n_bins=1086, nnz=120_000, n_sub=3, seed=2014, contig_weights=(6.8, 6.2, 5.3, 4.6, 4.0, 3.4, 2.7),
                                  mean_len_bp=660.0 * 9, accu=9, param=par)
    P = synth.make_problem(n_bins=90, nnz=2500, n_sub=3, seed=17, contig_weights=(5, 4, 3), mean_len_bp=2000.0, accu=9,
                           param=par, grid_bp=2000)
    if which == "sub3mix":
        # nine bins of mixed RF counts (a pyramid's ragged last bins): a commit that mirrors one of them reports its own-pixel correction as
        # unknown, and the step that follows evaluates in full -- on several ranks with the contacts' part summed over their shards
        acc = P["np_sub_frags_accu"].copy()
        acc[[3, 11, 17, 29, 37, 44, 61, 73, 88], 0] = 5
        P["np_sub_frags_accu"] = acc
    return P


def _make(P, rng, group, exchange=None):
    from graal_amd.sampler import sampler
    return sampler(True, P["S_o_A_frags"], P["collector_id_repeats"], P["frag_dispatcher"], P.get("id_frag_duplicated", []), [], P["n_frags"],
                   P["n_new_frags"], P["init_n_sub_frags"], P["n_new_sub_frags"], None,
                   (P["bin_coo_row"], P["bin_coo_col"], P["bin_coo_val"]), P["np_sub_frags_len_bp"], P["np_sub_frags_id"],
                   P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"], None, None,
                   (P["coo_row"], P["coo_col"], P["coo_val"]), P["mean_value_trans"], 1, False, None,
                   device=0, rng=rng, group=group, param_simu=P["param_simu"], compute_dist=False, exchange=exchange)


def _run(group, exchange=None, which="sub3", expect_repeat=False, counters=None):
    from graal_amd import em
    P = _problem(which)
    rng = np.random.RandomState(5)
    want = exchange
    if exchange == "auto-fallback":
        # the collective self-test of the shared segment fails on ONE rank: every rank must fall back to the all-reduce
        import warnings
        from graal_amd.lib import Engine
        real = Engine.exchange_selftest
        Engine.exchange_selftest = lambda self, tag, phase: real(self, tag, phase) and not (phase == 1 and group.rank == 1)
        warnings.simplefilter("ignore")
        exchange, want = "auto", "rccl"
    g = _make(P, rng, group, exchange)
    assert g.exchange == ("none" if group.world == 1 else want)
    scores = []
    # ("mid": from the map's own ten contigs of ~50 bins, not from the exploded genome: affected sets of ~100 fragments from the first step)
    t = em.run_em(g, 1, 4, rng=rng, scrambled=which != "mid", on_step=lambda j, i, tr: scores.append(np.copy(g.score)))
    if which == "mid":
        assert max(t.n_contigs) < 60, "the run left the regime of contigs of tens to hundreds of bins"
    if expect_repeat:     # (on the rank whose wait ran out AND on its peers, which repeated the step with it)
        assert g.engine.run_counters()["fallbacks"] >= 1, "no step was repeated on rank %d" % group.rank
    if which == "sub3mix" and g._own_corr:
        assert g.engine.run_counters()["carried_totals_repaired"] > 0, "no commit mirrored a bin of mixed RF counts: the case tests nothing"
    if counters is not None:
        counters.update(g.engine.run_counters())
    g.gpu_vect_frags.copy_from_gpu()
    out = (t.mutations(), np.concatenate(scores), {k: np.copy(v) for k, v in g.gpu_vect_frags.as_dict().items()},
           g.eval_likelihood())
    g.free_gpu()
    return out


def _worker(rank, world, port, q, exchange, which="sub3", scan_path=None):
    import torch.distributed as td
    from graal_amd import dist as gdist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    if scan_path is not None:      # (read when the engine is created: 0 the engine's own choice, 1 streaming, 2 through the row index)
        os.environ["GRAAL_SCAN_PATH"] = str(scan_path)
    expect_repeat = which.endswith("+timeout")
    if which.endswith("+timeout"):
        # ONE rank's in-kernel wait for its scan runs out at once (the engine reads the bound when the handle is created): its step ends as
        # failed and is repeated behind events -- and every other rank has to repeat that step with it
        which = which[:-len("+timeout")]
        if rank == 1:
            os.environ["GRAAL_TM_SPIN_TICKS"] = "1"
    td.init_process_group("gloo", rank=rank, world_size=world)
    try:
        rc = {}
        mut, scores, soa, full = _run(gdist.Group(rank, world), exchange, which, expect_repeat, counters=rc)
        q.put((rank, mut, scores, soa, full, rc))
    finally:
        td.destroy_process_group()


_REF = {}


def _ref(which, per_step_evaluation):
    """The one-rank anchor of a run.  With sub-fragments one rank -- and several ranks over the host exchange -- carry the total with the
    commits' own-pixel corrections (tests/test_carried_total_gpu.py); ranks behind an all-reduce evaluate the full likelihood every step, as
    the reference does: their bit-for-bit anchor is the one-rank run that does the same (GRAAL_NO_OWN_PIXEL_CARRY=1)."""
    from graal_amd import dist as gdist
    several_ranks = bool(per_step_evaluation) and which in ("sub3", "sub3mix", "c2")      # (the other problems never carry: one anchor)
    key = (which, several_ranks)
    if key not in _REF:
        if several_ranks:
            os.environ["GRAAL_NO_OWN_PIXEL_CARRY"] = "1"
        try:
            _REF[key] = _run(gdist.Group(0, 1), which=which)
        finally:
            os.environ.pop("GRAAL_NO_OWN_PIXEL_CARRY", None)
    return _REF[key]


@pytest.mark.timeout(900)
@pytest.mark.parametrize("world,exchange,which", [(2, "host", "sub3"), (3, "host", "sub3"), (2, "rccl", "sub3"), (2, "auto-fallback", "sub3"),
                                                  (2, "host", "mid"), (3, "host", "mid"), (2, "rccl", "mid"),
                                                  (2, "host", "rep"), (3, "host", "rep"), (2, "rccl", "rep"), (2, "host", "sub3mix"),
                                                  (2, "host", "sub3+timeout"), (3, "host", "mid+timeout"), (2, "host", "c2")])
def test_ranks_reproduce_the_single_rank_run_bit_for_bit(world, exchange, which):
    import torch.multiprocessing as mp
    from graal_amd import dist as gdist
    ref_mut, ref_scores, ref_soa, ref_full = _ref(which.replace("+timeout", ""), per_step_evaluation=exchange != "host")
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, exchange, which)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=500) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, mut, scores, soa, full, _ in res:
        assert np.array_equal(mut, ref_mut), rank
        assert np.array_equal(scores, ref_scores), rank          # bit-identical float64 scores
        for k in ref_soa:
            assert np.array_equal(soa[k], ref_soa[k]), (rank, k)
        assert full == ref_full


def _rank_child(rank, world, port, exchange, which, scan_path, out_path):
    """(one rank as a process of its own, started under `timeout`: what _worker puts into its queue goes to a file)"""
    import pickle

    class ToFile:
        def put(self, item):
            with open(out_path, "wb") as f:
                pickle.dump(item, f)

    _worker(rank, world, port, ToFile(), exchange, which, scan_path)


def _ranks(world, exchange, which, scan_path, tmp_path):
    """What `world` ranks on this GPU leave behind, by rank; every rank a child under a time limit of its own."""
    import pickle
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "GRAAL_SCAN_PATH", "GRAAL_SCAN_ROWS_R")}
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    outs = [str(tmp_path / ("rank%d.pkl" % r)) for r in range(world)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, "-c", "import tests.test_multirank_gpu as t; t._rank_child(%d, %d, %d, %r, %r, %r, %r)"
                               % (r, world, port, exchange, which, scan_path, outs[r])], cwd=root, env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(world)]
    said = [p.communicate()[0] for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, (r, p.returncode, said[r][-3000:])
    res = []
    for path in outs:
        with open(path, "rb") as f:
            res.append(pickle.load(f))
    return sorted(res, key=lambda r: r[0])


def _shards(which, world):
    """The ranks' shards of a problem's list, from numpy alone: (index arrays, rows split between ranks, per rank the rows it holds nothing of)."""
    from graal_amd import dist as gdist
    from tests import scan_rows_reference as R
    row = _problem(which)["coo_row"]
    ix = [gdist.shard_take(len(row), r, world) for r in range(world)]
    split, absent = R.split_rows(row, ix)
    return ix, split, absent


def _same_as_the_anchor(res, ref):
    ref_mut, ref_scores, ref_soa, ref_full = ref
    for rank, mut, scores, soa, full, _ in res:
        assert np.array_equal(mut, ref_mut), rank
        assert np.array_equal(scores, ref_scores), rank          # bit-identical float64 scores
        for k in ref_soa:
            assert np.array_equal(soa[k], ref_soa[k]), (rank, k)
        assert full == ref_full


@pytest.mark.timeout(600)
@pytest.mark.parametrize("scan_path", [2, 0])
@pytest.mark.parametrize("world,exchange,which", [(2, "host", "mid"), (2, "host", "sub3"), (2, "rccl", "mid")])
def test_ranks_with_a_row_index_over_their_own_shard(world, exchange, which, scan_path, tmp_path):
    """Every rank indexes ITS shard of the (row, col)-sorted list -- blocks of 4,096 contacts dealt round robin (graal_amd.dist.shard_take): a
    row can be split between ranks or be absent from one ("mid": tests/test_scan_rows_reference_cpu.py shows both) -- and finds a step's
    contacts through it: forced (GRAAL_SCAN_PATH=2: every evaluation of every rank is indexed) or by its own choice (0).  Bit for bit the
    one-rank anchor of the run, which chooses for itself over the whole list."""
    ix, split, absent = _shards(which, world)
    if which == "mid":        # 15,000 contacts: rank 0 holds blocks 0 and 2, rank 1 blocks 1 and 3 -- three rows are cut by a block boundary
        assert all(len(i) > 4096 for i in ix) and len(split) >= 1 and all(len(a) >= 1 for a in absent)
    else:                     # 2,500 contacts: one block -- rank 1 holds nothing, and its index is the empty list's
        assert len(ix[0]) == 2500 and len(ix[1]) == 0
    res = _ranks(world, exchange, which, scan_path, tmp_path)
    _same_as_the_anchor(res, _ref(which, per_step_evaluation=exchange != "host"))
    for rank, _, _, _, _, rc in res:
        assert rc["fallbacks"] == 0, (rank, rc)
        if exchange == "host":
            assert rc["evaluations"] >= 50, (rank, rc)
            if scan_path == 2:
                assert rc["indexed_passes"] == rc["evaluations"], (rank, rc)
        elif scan_path == 2:
            # (`evaluations` counts the synchronous entry point, which the all-reduce flow does not go through: 0 there.  A forced indexed
            # evaluation is indexed or an error, so the ranks' counts are the steps that evaluated -- the same on every rank)
            assert rc["indexed_passes"] >= 50 and rc["indexed_passes"] == res[0][5]["indexed_passes"], (rank, rc)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("scan_path", [0, 2])
def test_a_rank_with_an_empty_shard(scan_path, tmp_path):
    """Three ranks on a list of 6,000 contacts: rank 0 holds one block of 4,096, rank 1 the rest, rank 2 nothing.  An empty list is a sorted
    list: its row index is all zeros, every row's slice is empty.  By its own choice the empty rank never takes it (0 contacts are never 16
    times the bound) and streams over nothing; forced, its indexed pass queues nothing.  Either way the run is the one-rank run."""
    ix, split, absent = _shards("mid6k", 3)
    assert [len(i) for i in ix] == [4096, 6000 - 4096, 0] and len(split) == 1      # (the row the block boundary cuts)
    res = _ranks(3, "host", "mid6k", scan_path, tmp_path)
    _same_as_the_anchor(res, _ref("mid6k", per_step_evaluation=False))
    for rank, _, _, _, _, rc in res:
        assert rc["evaluations"] >= 50 and rc["fallbacks"] == 0, (rank, rc)
        if scan_path == 2:
            assert rc["indexed_passes"] == rc["evaluations"], (rank, rc)
    if scan_path == 0:
        assert res[2][5]["indexed_passes"] == 0


def _rccl_child(out_path, which):
    """(a child process: RCCL initialises once per process and GPU)"""
    from graal_amd import dist as gdist
    mut, scores, soa, full = _run(gdist.Group(0, 1), which=which)
    np.savez(out_path, mut=np.asarray(mut), scores=scores, full=full, **{"soa_" + k: v for k, v in soa.items()})


@pytest.mark.timeout(900)
@pytest.mark.parametrize("which", ["sub3", "mid"])
def test_rccl_all_reduce_driven_by_the_library_on_the_gpu_timeline(which, tmp_path):
    """exchange="rccl" as north_star words it -- one RCCL all-reduce of the per-shard logL vector per MCMC step -- driven by the library:
    the finishing kernel leaves the sums in a device buffer, ncclAllReduce runs on the engine's stream, a last kernel publishes the total,
    graal_step waits once (graal_attach_rccl).  One GPU cannot hold two RCCL ranks, so the FLOW is exercised with a one-rank
    communicator (GRAAL_RCCL_FORCE): every step goes device buffer -> all-reduce -> publication, and must reproduce the plain
    single-rank run bit for bit -- scores, trace, layout, full likelihood.  (What several ranks add -- the sharding -- is covered with the
    host exchange and with torch's all-reduce above; several RCCL ranks need several GPUs: the driver's scaling run.)"""
    import subprocess
    import sys
    from graal_amd import dist as gdist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ref_mut, ref_scores, ref_soa, ref_full = _ref(which, per_step_evaluation=False)   # (a one-rank communicator: the child carries its total like any single rank)
    out = str(tmp_path / "rccl.npz")
    env = dict(os.environ, GRAAL_RCCL_FORCE="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", "import tests.test_multirank_gpu as t; t._rccl_child(%r, %r)" % (out, which)], cwd=root, env=env,
                       capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    assert np.array_equal(got["mut"], np.asarray(ref_mut))
    assert np.array_equal(got["scores"], ref_scores)
    assert float(got["full"]) == ref_full
    for k in ref_soa:
        assert np.array_equal(got["soa_" + k], ref_soa[k]), k


@pytest.mark.timeout(900)
def test_bench_runs_two_ranks_from_one_command():
    """`python bench.py --gpus 2 --full` (no torchrun around it) on a small map: the launcher starts both ranks (here both on this
    one GPU, gloo instead of RCCL), rank 0 prints the one JSON line with both exchanges and the late-stage extra."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["GRAAL_BENCH_PHASES"] = "1"    # (where the run is, on stderr: shown if it fails)
    env["GRAAL_DEBUG_ADDR"] = "1"      # (... and where the engines' buffers are: a fault's address can be matched to one)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--full", "--backend", "gloo", "--n-bins", "2000",
           "--nnz", "100000", "--steps", "6", "--warmup", "2", "--mcmc-warmup", "300"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=400)
    if out.returncode != 0:      # (keep everything the ranks said -- phase markers, the engines' buffer map: gpurun_out/ travels back from the GPU box.
        # This rehearsal died of a GPU memory fault about one run in five until round 5 found the cause with exactly these diagnostics:
        # graal_layout_stats behind a commit made the next relabel count from the wrong number of contigs -- DESIGN.md section 9)
        try:
            os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
            with open(os.path.join(root, "gpurun_out", "bench_two_ranks_failure.log"), "a") as f:
                f.write("returncode %d\n--- stdout\n%s\n--- stderr\n%s\n" % (out.returncode, out.stdout, out.stderr))
        except OSError:
            pass
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["distributed"]["ranks"] == 2
    assert d["exchange_alt"]["value"] > 0 and "error" not in d["late_stage"]
    assert d["roofline"]["launches_timed"] >= 1
