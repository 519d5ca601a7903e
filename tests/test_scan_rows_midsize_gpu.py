"""GPU: the indexed contact producer (k_scan_rows) at the shapes where its control flow branches -- rows of exactly 0 .. 1,025 contacts (the
lanes' edge, the second and the third trip of the c0 loop), more affected rows than the grid has waves (the round robin), a full row list
(the block-wide prefix at ROWS_CAP, the host's refusal one past it), more bitmap words than threads -- and after a second upload on one
engine.

Every case (tests/scan_rows_cases.py) runs the same evaluations with graal_set_scan_path(1) and (2) on one engine, through
tests/test_scan_rows_gpu.both_paths: the deltas are np.array_equal, counters [1] and [2] are equal and equal the older numpy count, the
indexed run's `indexed_passes` grows by the number of evaluations, `fallbacks` stays.  On top of that, here, the count equals the count of
tests/scan_rows_reference.py -- the restatement of the pass itself -- and, BEFORE anything is launched, that reference's shape facts show
that the case reaches the branch it is named for (scan_rows_cases.get).  tests/test_scan_rows_reference_cpu.py shows on the CPU that the
reference with the matching flaw built in -- a second trip never taken, a second row never taken, one word per thread, the end of a full
list lost, a slice one short -- misses the true count of the same case.

One case is anchored outside the engine: the indexed deltas of the exact-row-lengths layout in reference arithmetic against the numpy
re-score (oracle/sparse_numpy.py), to tests/test_independent_checker_gpu.py's own tolerance, and against the dense C restatement of the reference
(oracle.DenseOracle)."""
import numpy as np
import pytest

from tests import scan_rows_cases as C
from tests import scan_rows_reference as R
from tests.test_scan_rows_gpu import INDEXED, STREAM, both_paths, engine_for, set_arithmetic

pytestmark = pytest.mark.gpu


def run_case(name, which):
    case, refs = C.get(name)
    for ref in refs:      # a forced indexed evaluation never lists more rows than the kernel's list holds
        assert ref["shape"]["bound"] <= R.ROWS_CAP and ref["shape"]["n_rows"] <= R.ROWS_CAP
    P, s = case["P"], case["state"]
    e = engine_for(P, s)
    set_arithmetic(e, which)
    max_id = e.relabel_contigs()
    got = both_paths(e, P, s, case["evals"], max_id)
    for ref, a, b in zip(refs, got[STREAM], got[INDEXED]):
        assert ref["count"] >= 1 and b[2] == ref["count"] and b[1] == ref["count"] and a[2] == ref["count"]
    e.close()
    return case, refs


@pytest.mark.parametrize("which", ["exact", "strict"])
@pytest.mark.parametrize("n_sub", [1, 3])
def test_rows_of_exact_lengths_around_the_lanes_and_the_trips(n_sub, which):
    """Rows of 0, 1, 64, 65, 511, 512, 513, 1,024 and 1,025 contacts (three sub-fragments per bin: 0, 1, 65, 512, 513, 1,025) in two contigs
    of a few hundred fragments, K = 1 and K = 3: rows that take a second and a third trip, each of them queueing its last contact."""
    case, refs = run_case("exact_row_lengths-%d" % n_sub, which)
    assert all(r["shape"]["rows_over_512"] >= 2 and r["shape"]["rows_over_1024"] >= 1 for r in refs)


@pytest.mark.parametrize("n_sub", [1, 3])
def test_a_full_row_list(n_sub):
    """Two contigs of 1,024 fragments (341 bins of three sub-fragments): the bound is 2,048 (2,046), the list is full, every wave makes 8 trips."""
    case, refs = run_case("at_the_cap-%d" % n_sub, "strict")
    assert refs[0]["shape"]["bound"] == (2048 if n_sub == 1 else 2046) and refs[0]["shape"]["trips_per_wave"] == 8
    if n_sub == 1:
        assert refs[0]["shape"]["n_rows"] == R.ROWS_CAP


@pytest.mark.parametrize("n_sub", [1, 3])
def test_one_past_the_cap_is_refused_and_streams(n_sub):
    """The same with one contig one longer (1,025 fragments; 342 bins): the host refuses a forced indexed pass before it launches anything, and
    the engine's own choice streams.  (A refusal test: the kernel's own overflow branch stays out of reach.)"""
    from graal_amd.lib import GraalError
    case, refs = C.get("one_past_the_cap-%d" % n_sub)
    assert refs[0]["shape"]["bound"] == (2050 if n_sub == 1 else 2052) > R.ROWS_CAP
    P, s = case["P"], case["state"]
    (fA, fBs), = case["evals"]
    e = engine_for(P, s)
    set_arithmetic(e, "strict")
    max_id = e.relabel_contigs()
    e.set_scan_path(STREAM)
    want = e.eval_candidates(fA, fBs, max_id)
    assert int(e.last_counters()[2]) == refs[0]["count"]
    before = e.run_counters()
    e.set_scan_path(INDEXED)          # (the list has an index: the path can be asked for ...)
    with pytest.raises(GraalError, match="too long"):
        e.eval_candidates(fA, fBs, max_id)      # (... but not for this step)
    assert e.run_counters()["indexed_passes"] == before["indexed_passes"]
    e.set_scan_path(0)
    got = e.eval_candidates(fA, fBs, max_id)
    after = e.run_counters()
    assert np.array_equal(got, want) and int(e.last_counters()[2]) == refs[0]["count"]
    assert after["indexed_passes"] == before["indexed_passes"] and after["fallbacks"] == before["fallbacks"]
    e.close()


@pytest.mark.parametrize("n_sub", [1, 3])
def test_more_rows_than_waves(n_sub):
    """K = 5, contigs of 60-120 fragments: 64 blocks, 256 waves, 555 (1,530) rows -- every wave takes a second row, the list is far from full."""
    case, refs = run_case("round_robin-%d" % n_sub, "strict")
    assert all(r["shape"]["grid"] == 64 and r["shape"]["trips_per_wave"] >= 2 and r["shape"]["bound"] > 256 for r in refs)


@pytest.mark.parametrize("n_sub", [1, 3])
def test_more_bitmap_words_than_threads(n_sub):
    """9,001 ids (not a multiple of 32) and about 9,000 ids in 3,000 bins: two bitmap words per thread; affected ids in the first, a middle and the
    last word, the very last id among them."""
    case, refs = run_case("many_words-%d" % n_sub, "strict")
    assert all(r["shape"]["words_per_thread"] == 2 for r in refs)


def _anchor_sampler():
    import bench
    case, refs = C.get("exact_row_lengths-1")
    P = dict(case["P"], S_o_A_frags=case["state"])
    smp = bench.build_sampler(P, np.random.RandomState(86), None, 0)
    assert smp.reference_arithmetic == "strict"
    smp.init_likelihood()
    smp.engine.set_timing(0)
    smp.engine.set_scan_path(INDEXED)
    return case, refs, P, smp


def test_indexed_deltas_against_the_numpy_rescore():
    """The anchor outside the engine: on the exact-row-lengths layout, in reference arithmetic, the deltas the INDEXED pass leads to against
    re-score(candidate) - re-score(current) of the numpy sparse re-score, for the 13 candidates of each neighbour of a K = 1 and a K = 3
    proposal, to tests/test_independent_checker_gpu.py's own tolerance (1e-8 x |logL|).

    One candidate here, (fA 1210, fB 53, operation 10), closes a ring of 187 fragments whose cis mass, 286,563, is a third of
    |logL| = 918,975.77: the re-score's float32 pow and exp have to be good to 3e-8 of that mass.  With numpy's own float32 functions they
    were not (the re-score was 6.76e-8 x |logL| from the engine AND from the dense restatement, which agreed); oracle/sparse_numpy.py now
    rounds the float64 functions once, as a C powf / expf does to within the rare double rounding, and agrees with the dense restatement to
    5.5e-13 x |logL| on all 52 candidates."""
    from tests.test_independent_checker_gpu import check_against_the_numpy_rescore
    case, refs, P, smp = _anchor_sampler()
    e = smp.engine
    proposals = [(int(fA), [int(f) for f in fBs]) for fA, fBs in case["evals"]]
    before = e.run_counters()
    try:
        worst, full_err, n_c = check_against_the_numpy_rescore(P, smp, proposals)
        after = e.run_counters()
        print("exact row lengths, indexed: %d candidates, worst |delta - numpy re-score| / |logL| = %.2e, full evaluation %.2e" % (n_c, worst, full_err))
        assert n_c >= 2 * 13
        assert after["indexed_passes"] - before["indexed_passes"] == len(proposals) and after["fallbacks"] == before["fallbacks"]
        assert int(e.last_counters()[2]) == refs[-1]["count"]
    finally:
        smp.free_gpu()


def test_indexed_deltas_against_the_dense_restatement():
    """The same layout and proposals, the indexed pass forced, against the dense C restatement of the reference's kernels run the reference's way
    (oracle.DenseOracle, every pixel of the 2,600 x 2,600 map): the full evaluation to 1e-8 x |logL| and all 13 x 4 candidate deltas to
    2e-9 x |logL| -- the bounds of the smoke run's reference-arithmetic leg."""
    from graal_amd import synth
    from oracle import oracle as O
    from tests import util
    from tests.test_independent_checker_gpu import _layout
    case, refs, P, smp = _anchor_sampler()
    e = smp.engine
    max_id = int(smp.modify_gl_cuda_buffer(0))
    cur = _layout(smp)
    Pd = synth.with_dense(P)
    dense = O.DenseOracle(Pd["hic_matrix"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["frag_dispatcher"],
                          P["collector_id_repeats"], P["n_frags"], P["mean_squared_frags_per_bin"], P["param_simu"], fix_trans_accu=False)
    per_pix = np.zeros(dense.n_pix)
    base = dense.evaluate(cur, per_pix)
    assert abs(smp._full_likelihood() - base) <= 1e-8 * abs(base)
    before = e.run_counters()
    worst, n_c = 0.0, 0
    for (fA, fBs), ref in zip(case["evals"], refs):
        got = smp._candidate_deltas(int(fA), [int(f) for f in fBs], max_id)
        assert int(e.last_counters()[2]) == ref["count"]
        for k, fB in enumerate(fBs):
            sub = np.sort(np.nonzero((cur["id_c"] == cur["id_c"][fA]) | (cur["id_c"] == cur["id_c"][fB]))[0])
            for op in range(13):
                cand, stale = util.oracle_candidate(cur, int(fA), int(fB), op, max_id)
                if stale:
                    continue
                want = dense.sub_compute(cand, sub, [], np.arange(P["n_frags"], dtype=np.int32), per_pix)
                err = abs(got[k, op] - want) / abs(base)
                assert err <= 2e-9, (fA, int(fB), op, got[k, op], want, err)
                worst, n_c = max(worst, err), n_c + 1
    after = e.run_counters()
    print("exact row lengths, indexed: %d candidates, worst |delta - dense restatement| / |logL| = %.2e" % (n_c, worst))
    assert n_c >= 2 * 13
    assert after["indexed_passes"] - before["indexed_passes"] == len(case["evals"]) and after["fallbacks"] == before["fallbacks"]
    smp.free_gpu()


def test_a_second_and_a_third_upload_on_one_engine():
    """sorted -> unsorted -> another sorted list on one handle: the row index is freed and rebuilt, graal_set_scan_path keeps its value."""
    from graal_amd.lib import GraalError
    case, refs = C.get("round_robin-1")
    P, s, evals = case["P"], case["state"], case["evals"]
    e = engine_for(P, s)
    ref_engine = engine_for(P, s)        # (the sorted engine the streamed deltas of the permuted list are held against)
    max_id = e.relabel_contigs()
    assert ref_engine.relabel_contigs() == max_id
    both_paths(e, P, s, evals, max_id)
    ref_engine.set_scan_path(STREAM)
    want = [ref_engine.eval_candidates(fA, fBs, max_id) for fA, fBs in evals]
    e.set_scan_path(INDEXED)
    # ---- a permuted list: no index; the forced path is kept and the next evaluation says why it cannot be had
    rng = np.random.RandomState(87)
    perm = rng.permutation(len(P["coo_row"]))
    e.upload_contacts(P["coo_row"][perm], P["coo_col"][perm], P["coo_val"][perm])
    before = e.run_counters()
    with pytest.raises(GraalError, match="row index|sorted"):
        e.eval_candidates(evals[0][0], evals[0][1], max_id)
    e.set_scan_path(0)
    for (fA, fBs), w, ref in zip(evals, want, refs):
        assert np.array_equal(e.eval_candidates(fA, fBs, max_id), w)
        assert int(e.last_counters()[2]) == ref["count"]
    assert e.run_counters()["indexed_passes"] == before["indexed_passes"]
    with pytest.raises(GraalError, match="row index|sorted"):
        e.set_scan_path(INDEXED)
    # ---- another sorted list (the exact-row-lengths map: the same ids, other contacts): indexed again, the counts are the new list's
    P2 = C.get("exact_row_lengths-1")[0]["P"]
    assert len(P2["coo_row"]) != len(P["coo_row"]) and np.array_equal(P2["bin_of_sub"], P["bin_of_sub"])
    e.upload_contacts(P2["coo_row"], P2["coo_col"], P2["coo_val"])
    refs2 = [R.indexed_pass(P2["coo_row"], P2["coo_col"], P2["bin_of_sub"], s["id_c"], fA, fBs, int(s["l_cont"].max())) for fA, fBs in evals]
    assert all(r["count"] >= 1 for r in refs2) and [r["count"] for r in refs2] != [r["count"] for r in refs]
    got = both_paths(e, P2, s, evals, max_id)
    for ref, b in zip(refs2, got[INDEXED]):
        assert b[2] == ref["count"]
    e.close()
    ref_engine.close()
