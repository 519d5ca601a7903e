"""CPU: the numpy restatement of the indexed contact producer (tests/scan_rows_reference.py) pinned against what is independent of it --
the older numpy count of tests/test_scan_rows_gpu.py (np.isin over both ends of every contact: no slices, no searchsorted), and the
host's own row index, bound and switch (graal_amd/csrc/scan_rows.h through the test-only host library) --, and every case of
tests/scan_rows_cases.py checked for reaching the part of the kernel it is named for.

For each case the reference is also run with the `flaw` the case is built to expose -- a slice that ends one contact early, a c0 loop that
never takes a second trip, a wave that never takes a second row, a listing of one bitmap word per thread, a prefix that loses the end of a
full list -- and its count must then differ from the true count: the comparison the GPU test makes would fail on a kernel with that flaw."""
import numpy as np
import pytest

from graal_amd import dist as gdist
from tests import scan_rows_cases as C
from tests import scan_rows_reference as R
from tests import test_scan_rows_gpu as G
from tests.test_scan_rows_cpu import hc, row_index


@pytest.mark.parametrize("n_sub,seed,n_bins,nnz,n_contigs", [(1, 71, 400, 30000, 150), (3, 72, 240, 40000, 90), (1, 73, 300, 30000, 20),
                                                            (3, 73, 300, 30000, 20), (1, 75, 300, 30000, 110), (1, 76, 400, 40000, 140)])
def test_reference_equals_the_older_numpy_count_and_the_hosts_index(n_sub, seed, n_bins, nnz, n_contigs):
    P = G.make(n_sub, seed, n_bins, nnz, accu=("random", 3, 12) if seed == 72 else None)
    rng = np.random.RandomState(seed)
    s = G.layout(P, rng, n_contigs)
    S = int(P["init_n_sub_frags"])
    srt, longest, rowptr = row_index(P["coo_row"], S)
    assert srt
    L = hc()
    for f in rng.choice(P["n_frags"], 8, replace=False):
        for K in (1, 5, 10):
            nb = G.map_neighbours(P, int(f), K, rng)
            ref = R.indexed_pass(P["coo_row"], P["coo_col"], P["bin_of_sub"], s["id_c"], int(f), nb, int(s["l_cont"].max()))
            assert ref["count"] == G.numpy_count(P, s, int(f), nb) >= 1
            assert np.array_equal(ref["lo"], rowptr[ref["ids"]]) and np.array_equal(ref["hi"], rowptr[ref["ids"] + 1])
            assert np.all(np.diff(ref["ids"]) > 0) and np.all(np.diff(ref["queued"]) > 0)
            assert ref["per_row"].sum() == ref["count"]
            sh = ref["shape"]
            assert sh["bound"] == L.hc_scan_rows_bound(len(nb), int(s["l_cont"].max()), int(n_sub == 1))
            assert sh["n_rows"] <= sh["bound"] and sh["longest_row"] <= longest
            for n_list in (nnz, 16 * sh["bound"] * longest, 16 * sh["bound"] * longest - 1):
                assert R.switch_takes_index(sh, longest, n_list) == bool(L.hc_scan_rows_wins(sh["bound"], longest, n_list, R.SWITCH_R))


def test_constants_and_shape_facts():
    assert hc().hc_scan_rows_cap() == R.ROWS_CAP
    sh = R.shape_facts(2048, [0, 1, 512, 513, 1024, 1025], 1, 1024, True, 2600)
    assert (sh["bound"], sh["grid"], sh["n_waves"], sh["trips_per_wave"]) == (2048, 64, 256, 8)
    assert (sh["rows_over_512"], sh["rows_over_1024"], sh["words_per_thread"]) == (3, 1, 1)
    sh = R.shape_facts(6, [3], 5, 1, True, 50000)                 # the benchmark's exploded layout
    assert (sh["bound"], sh["grid"], sh["trips_per_wave"], sh["words_per_thread"]) == (6, 2, 1, 7)
    assert R.shape_facts(300, [], 1, 341, False, 2700)["bound"] == 2046 and R.shape_facts(300, [], 1, 342, False, 2700)["bound"] == 2052
    assert R.shape_facts(1, [], 1, 1, True, 8192 - 64)["words_per_thread"] == 1 and R.shape_facts(1, [], 1, 1, True, 8192)["words_per_thread"] == 2


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_case_engages_what_it_is_named_for(name):
    case, refs = C.get(name)
    P, s = case["P"], case["state"]
    from tests import util
    util.check_invariants(s)
    S = int(P["init_n_sub_frags"])
    srt, longest, rowptr = row_index(P["coo_row"], S)
    keys = P["coo_row"].astype(np.int64) * S + P["coo_col"]
    assert srt and np.all(keys[1:] > keys[:-1])
    single = int(len(P["bin_of_sub"]) == P["n_frags"])
    for (fA, fBs), ref in zip(case["evals"], refs):
        assert np.array_equal(ref["lo"], rowptr[ref["ids"]]) and np.array_equal(ref["hi"], rowptr[ref["ids"] + 1])
        assert ref["shape"]["bound"] == hc().hc_scan_rows_bound(len(fBs), int(s["l_cont"].max()), single)
        assert len(set(int(f) for f in fBs)) == len(fBs) and list(fBs) == sorted(fBs)


@pytest.mark.parametrize("name", sorted(n for n in C.CASES if not n.startswith("one_past")))
def test_a_flawed_reference_misses_the_true_count(name):
    case, refs = C.get(name)
    for flaw in (case["flaw"],) + tuple(case.get("also_flaws", ())):
        bad = C._refs(case, flaw)
        for (fA, fBs), ref in zip(case["evals"], bad):
            true = G.numpy_count(case["P"], case["state"], fA, fBs)
            assert ref["count"] < true, (name, flaw, fA)


def test_the_switch_runs_map_starts_indexed_and_flips_between_4_and_64():
    """The sizing of test_scan_rows_gpu.switch_problem with the shipped ratio and K = 4 (what its run proposes)."""
    P = G.switch_problem()
    nnz, longest = len(P["coo_row"]), int(np.bincount(P["coo_row"]).max())
    assert (nnz, longest) == (1_000_000, 661)
    L = hc()
    takes = [bool(L.hc_scan_rows_wins(L.hc_scan_rows_bound(4, lc, 1), longest, nnz, R.SWITCH_R)) for lc in range(1, 200)]
    assert takes[4 - 1], "the exploded start (bound of the longest contig between relabels: 2 x 1 + 2) is not indexed"
    first_streamed = 1 + takes.index(False)
    assert first_streamed == 19 and 4 < first_streamed < 64 and not any(takes[first_streamed - 1:])
    for lc in (4, 18, 19, 64):
        assert R.switch_takes_index(R.shape_facts(0, [], 4, lc, True, 3000), longest, nnz) == takes[lc - 1]


def test_shards_of_the_multirank_cases_split_rows_and_leave_a_rank_empty():
    from tests.test_multirank_gpu import _problem
    for which in ("mid", "sub3"):
        P = _problem(which)
        nnz = len(P["coo_row"])
        if nnz > 4096:
            shards = [gdist.shard_take(nnz, r, 2) for r in range(2)]
            split, absent = R.split_rows(P["coo_row"], shards)
            assert len(split) >= 1 and all(len(a) >= 1 for a in absent), which      # a row split between ranks, rows absent from a rank
            for ix in shards:
                assert len(ix) and np.all(np.diff(P["coo_row"][ix]) >= 0)           # every shard still sorted: it gets an index of its own
    P = _problem("mid6k")
    nnz = len(P["coo_row"])
    assert 4096 < nnz < 8192
    shards = [gdist.shard_take(nnz, r, 3) for r in range(3)]
    assert len(shards[0]) == 4096 and len(shards[1]) == nnz - 4096 and len(shards[2]) == 0
    split, absent = R.split_rows(P["coo_row"], shards)
    assert len(split) == 1                                                          # the row the block boundary cuts
