"""CPU: the oracle (oracle/graal_oracle.c) and the host build of the engine's frag_ops.h against the REFERENCE'S OWN
kernels, compiled for the host and run with a real block/thread/barrier model (oracle/ref_kernels.py, recipe in
oracle/Makefile, built by build() wherever the reference's sources are).

* live differential tests (skipped where the library could not be built): scalar model functions bit for bit, the 13
  candidates of every case of tests/ref_cases.py field by field, the full evaluation pixel by pixel, the candidate
  deltas, whole start_EM runs against tests/golden/traces.json;
* fixture tests (always run): the oracle and the host build of frag_ops.h reproduce tests/golden/ref_mutations.npz,
  ref_likelihood.npz and ref_likelihood_params.npz (four layouts under the parameter sets of tests/param_cases.py), which were
  recorded from the reference's kernels and are what the GPU tests read.

Bounds.  Integer results are equal.  float32 model values and per-pixel float64 log-likelihoods are equal as bit
patterns: both sides make the same libm calls in the same order (the table in oracle/ref_host/curand_kernel.h).  Sums
over pixels differ only in the order of the additions (the kernels: per thread, then per block; the oracle: in
sequence), so two sums of the same N terms t_i are held to N * 2^-53 * sum |t_i|.
"""
import json
import os

import numpy as np
import pytest

from graal_amd import em, synth
from oracle import oracle as O
from oracle import ref_kernels as R
from tests import param_cases
from tests import ref_cases as C
from tests import util
from tests.golden.make_traces import problem as trace_problem
from tests.test_oracle_golden import toy_likelihood_problem

HERE = os.path.dirname(os.path.abspath(__file__))
needs_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref/libgraal_ref.so needs the reference's kernels3.cu")
TRACES = json.load(open(os.path.join(HERE, "golden", "traces.json")))
APPENDIX_E = json.load(open(os.path.join(HERE, "golden", "appendix_e.json")))
MUT = np.load(os.path.join(HERE, "golden", "ref_mutations.npz"))
LIK = np.load(os.path.join(HERE, "golden", "ref_likelihood.npz"))
LIK_PARAMS = np.load(os.path.join(HERE, "golden", "ref_likelihood_params.npz"))


def bits32(x):
    return np.asarray(x, np.float32).view(np.uint32)


def bits64(x):
    return np.asarray(x, np.float64).view(np.uint64)


def sum_bound(terms):
    terms = np.asarray(terms, np.float64)
    return terms.size * 2.0 ** -53 * np.abs(terms).sum()


def appendix_e_param():
    p = APPENDIX_E["likelihood_toy"]["param_simu"]
    c1 = np.float32(0.53 * 9.6 ** -1.5)
    return np.array([p["kuhn"], p["lm"], c1, p["slope"], p["d"], p["d_max"], p["fact"], p["v_inter"]], np.float32)


PARAM_SETS = {"synth_defaults": synth.make_param_simu(), "appendix_e": appendix_e_param(),
              "case_layouts": synth.make_param_simu(fact=300.0, v_inter=0.03)}
# the sets a fit or a nuisance step gives (tests/param_cases.py), at the case layouts' fact and v_inter: kuhn != 1, other slopes, d <= 2
PARAM_SETS.update({name: param_cases.param(name, PARAM_SETS["case_layouts"]) for name in param_cases.NAMES})
# (layout, parameter set) of the live likelihood tests: every layout under its own parameters, four of them under the two fitted sets
LIVE = [(li, None) for li in range(len(C.LAYOUTS))] + [(li, name) for li in C.PARAM_LAYOUT_INDEX for name in param_cases.FITTED]
LIVE_IDS = [C.LAYOUTS[li]["name"] + ("-" + name if name else "") for li, name in LIVE]
RECORDED = [(li, name) for li in C.PARAM_LAYOUT_INDEX for name in param_cases.NAMES]
RECORDED_IDS = ["%s-%s" % (C.LAYOUTS[li]["name"], name) for li, name in RECORDED]


def live_layout(li, name):
    return C.LAYOUTS[li] if name is None else C.layout_under(li, name)


# ---- the case list itself ---------------------------------------------------------------------------------------------------
def test_case_list_covers_every_class():
    assert all(C.CLASS_COUNTS[c] >= 8 for c in C.CLASSES), C.CLASS_COUNTS
    assert len(C.PAIRS) == sum(C.K * len(lay["proposals"]) for lay in C.LAYOUTS)
    lens = np.concatenate([lay["state"]["len_bp"] for lay in C.LAYOUTS])
    assert np.any(lens % 2000 != 0) and any(np.all(lay["state"]["len_bp"] % 2000 == 0) for lay in C.LAYOUTS)


def test_ref_kernels_refuses_the_corrected_indexing():
    lay = C.LAYOUTS[0]
    P = lay["P"]
    with pytest.raises(ValueError):
        R.RefKernels(P["hic_matrix"], P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"],
                     P["frag_dispatcher"], P["collector_id_repeats"], P["n_frags"], P["mean_squared_frags_per_bin"],
                     P["param_simu"], fix_trans_accu=True)


# ---- scalar functions ------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", sorted(PARAM_SETS))
def test_contact_model_bit_equal(name):
    p = np.asarray(PARAM_SETS[name], np.float32)
    d_max = np.float32(p[5])
    rng = np.random.RandomState(20)
    s = np.exp(rng.uniform(np.log(1e-3), np.log(2.0 * float(d_max)), 20000)).astype(np.float32)
    edges = np.array([0.0, d_max, np.nextafter(d_max, np.float32(0)), np.nextafter(d_max, np.float32(np.inf))], np.float32)
    s = np.concatenate([edges, s])
    s_tot = (s * rng.uniform(1.0, 4.0, len(s)) + rng.uniform(0.0, float(d_max), len(s))).astype(np.float32)
    got = np.array([O.rippe(x, p) for x in s], np.float32)
    want = np.array([R.rippe(x, p) for x in s], np.float32)
    assert np.array_equal(bits32(got), bits32(want)), np.nonzero(bits32(got) != bits32(want))[0][:10]
    # s = 0, s = d_max and one step above it are outside the window (kernels3.cu:125): the trans level
    assert np.unique(want).size > 1000 and want[0] == p[7] and want[1] == p[7] and want[3] == p[7]
    got = np.array([O.rippe_circ(x, t, p) for x, t in zip(s, s_tot)], np.float32)
    want = np.array([R.rippe_circ(x, t, p) for x, t in zip(s, s_tot)], np.float32)
    assert np.array_equal(bits32(got), bits32(want)), np.nonzero(bits32(got) != bits32(want))[0][:10]


@needs_ref
def test_pixel_likelihood_and_factorial_bit_equal():
    tiny = [np.nextafter(0.0, 1.0), float(np.finfo(np.float32).tiny), float(np.finfo(np.float64).tiny)]
    with np.errstate(all="ignore"):
        for ob in (0.0, 1.0, 9.0, 10.0, 14.0, 15.0, 16.0, 1000.0):
            for ex in [0.0, 1e-30, 1.0, 1e4] + tiny:
                assert bits64(O.lik(ex, ob)) == bits64(R.lik(ex, ob)), (ex, ob, O.lik(ex, ob), R.lik(ex, ob))
        rng = np.random.RandomState(21)
        for ex, ob in zip(np.exp(rng.uniform(-20, 10, 4000)), np.floor(np.exp(rng.uniform(0, 7, 4000)))):
            assert bits64(O.lik(ex, ob)) == bits64(R.lik(ex, ob)), (ex, ob)
        for n in list(range(0, 40)) + [0.5, 9.5, 9.999, 10.0, 14.7, 33.9, 34.0, 35.0, 170.0, -1.0]:
            assert bits32(O.factorial(n)) == bits32(R.factorial(n)), n
    assert R.factorial(5) == 120.0 and R.factorial(9.5) == 362880.0


# ---- mutations -------------------------------------------------------------------------------------------------------------
def assert_candidates_equal(got, want, where):
    (out_g, wr_g, st_g), (out_w, wr_w, st_w) = got, want
    assert np.array_equal(st_g, st_w), (where, st_g, st_w)
    assert np.array_equal(wr_g, wr_w), where
    assert np.array_equal(out_g, out_w), (where, np.argwhere(out_g != out_w)[:5])


def check_hostcheck_against(lay, fA, fB, out_ref, written_ref, stale_ref):
    """hc_apply_move (the host build of the engine's frag_ops.h) against the reference on the written entries; where the
    engine's ABI documents a refusal -- fA == fB is a no-op for the ten candidates that involve fB (DESIGN.md section 2,
    item 4) -- the refusal is asserted.  Returns the number of refused candidates."""
    s = lay["state"]
    refused = 0
    for op in range(C.N_OPS):
        got, n_stale = util.hc_apply_move(s, fA, fB, op, lay["max_id"])
        if fA == fB and op in C.OPS_NEEDING_FB:
            assert n_stale == 0 and all(np.array_equal(got[k], s[k]) for k in O.FIELDS), (lay["name"], fA, op)
            refused += 1
            continue
        assert n_stale == stale_ref[op], (lay["name"], fA, fB, op, n_stale, stale_ref[op])
        w = written_ref[op]
        for i, k in enumerate(O.FIELDS):
            assert np.array_equal(got[k][w], out_ref[op, i][w]), (lay["name"], fA, fB, op, k)
    return refused


@needs_ref
@pytest.mark.parametrize("li", range(len(C.LAYOUTS)), ids=[lay["name"] for lay in C.LAYOUTS])
def test_candidate_layouts_oracle_and_frag_ops_equal_the_reference(li):
    lay = C.LAYOUTS[li]
    refused = expected_refusals = 0
    for fA, fBs in lay["proposals"]:
        for fB in fBs:
            out_r, wr_r, st_r, ids_r = C.mutation_record(R.RefKernels, lay, fA, fB)
            out_o, wr_o, st_o, ids_o = C.mutation_record(O.DenseOracle, lay, fA, fB)
            assert_candidates_equal((out_o, wr_o, st_o), (out_r, wr_r, st_r), (lay["name"], fA, fB))
            for op in range(C.N_OPS):
                assert len(ids_o[op]) == len(ids_r[op]) == (1 if op <= 8 else 2)
                for a, b in zip(ids_o[op], ids_r[op]):
                    assert np.array_equal(a, b), (lay["name"], fA, fB, op)
            refused += check_hostcheck_against(lay, fA, fB, out_r, wr_r, st_r)
            expected_refusals += len(C.OPS_NEEDING_FB) if fA == fB else 0
    assert refused == expected_refusals


@needs_ref
@pytest.mark.parametrize("li", range(len(C.LAYOUTS)), ids=[lay["name"] for lay in C.LAYOUTS])
def test_single_kernels_equal_the_reference(li):
    """The kernels the 13 candidates do not reach alone: pop_in_frag_4, split_contig in both directions, and paste_contigs
    on the layout as it is (not behind two splits), each on a sentinel-filled output."""
    lay = C.LAYOUTS[li]
    s, n, max_id = lay["state"], len(lay["state"]["pos"]), lay["max_id"]

    def both(run):
        outs = []
        for D in (O.DenseOracle, R.RefKernels):
            out = O.new_state(n)
            for k in O.FIELDS:
                out[k][:] = C.SENTINEL
            ids = np.full(n, C.SENTINEL, np.int32)
            outs.append((out, ids, run(D, out, ids)))
        (a, ia, ra), (b, ib, rb) = outs
        assert ra == rb
        assert np.array_equal(ia, ib)
        for k in O.FIELDS:
            assert np.array_equal(a[k], b[k]), k

    for fA, fBs in lay["proposals"]:
        for fB in fBs:
            for up in (0, 1):
                both(lambda D, out, ids: D.split(out, s, ids, fA, up, max_id))
                both(lambda D, out, ids: D.split(out, s, ids, fB, up, max_id))
            both(lambda D, out, ids: D.paste(out, s, fA, fB, max_id))
            both(lambda D, out, ids: D.paste(out, s, fB, fA, max_id))
            for ori in (1, -1):
                def pop_in_4(D, out, ids):
                    pop = O.new_state(n)
                    D.pop_out(pop, s, ids, fA, max_id)
                    D.pop_in(4, out, pop, fA, fB, ids.max(), ori)
                both(pop_in_4)


# ---- likelihood ------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("li,params", LIVE, ids=LIVE_IDS)
def test_full_evaluation_per_pixel_bit_equal(li, params):
    lay = live_layout(li, params)
    pix_o, tot_o = C.likelihood_record(C.kernels_for(lay, O.DenseOracle), lay)
    pix_r, tot_r = C.likelihood_record(C.kernels_for(lay, R.RefKernels), lay)
    assert np.array_equal(bits64(pix_o), bits64(pix_r)), np.nonzero(bits64(pix_o) != bits64(pix_r))[0][:10]
    assert np.count_nonzero(pix_r) > len(pix_r) // 2
    assert abs(tot_o - tot_r) <= sum_bound(pix_r), (tot_o, tot_r)


@needs_ref
@pytest.mark.parametrize("li,params", LIVE, ids=LIVE_IDS)
def test_candidate_deltas_equal_the_reference(li, params):
    lay = live_layout(li, params)
    dev_o, dev_r = C.kernels_for(lay, O.DenseOracle), C.kernels_for(lay, R.RefKernels)
    per_pix, _ = C.likelihood_record(dev_r, lay)
    n_stale = 0
    for fA, fBs in lay["proposals"]:
        d_o, _ = C.delta_record(dev_o, O.DenseOracle, lay, per_pix, fA, fBs)
        d_r, bound = C.delta_record(dev_r, R.RefKernels, lay, per_pix, fA, fBs)
        assert np.array_equal(np.isnan(d_o), np.isnan(d_r))
        ok = ~np.isnan(d_r)
        n_stale += int((~ok).sum())
        assert np.all(np.abs(d_o - d_r)[ok] <= bound[ok]), (lay["name"], fA, fBs, np.abs(d_o - d_r)[ok].max())
        # only a candidate of fA with itself can be stale
        assert all(fBs[k] == fA for k in np.nonzero(~ok)[0])
        assert np.any(d_r[ok] != 0)


# ---- whole runs ------------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", sorted(TRACES))
def test_whole_runs_over_the_reference_kernels_reproduce_the_traces(name):
    g = TRACES[name]
    generic = g.get("generic", False)
    P = trace_problem(g["n_sub"], g["seed"], g["n_bins"], g["nnz"], g["blacklist"], g["repeats"], generic)
    if not generic:
        # the trace was made with fix_trans_accu=True: it is the reference's run only where the flag changes nothing,
        # that is where every sub-fragment of a bin carries the same RF count
        ids = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
        accu = np.asarray(P["np_sub_frags_accu"]).reshape(-1, 3)
        assert all(len(set(accu[b, :ids[b, 3]])) == 1 for b in range(len(ids)))
    else:
        accu = np.asarray(P["np_sub_frags_accu"]).reshape(-1, 3)
        assert any(len(set(row)) > 1 for row in accu)        # the run where the reference's indexing matters
    ora = O.OracleSampler(P, np.random.RandomState(g["seed"]), dev_class=R.RefKernels)
    t = em.run_em(ora, g["cycles"], g["neighbours"], rng=ora.rng)
    assert np.asarray(t.mutations()).tolist() == g["mutations"]
    assert [int(x) for x in t.n_contigs] == g["n_contigs"]
    assert [float(x) for x in t.dist] == g["dist"]
    assert np.allclose(t.likelihood, g["likelihood"], rtol=1e-12, atol=0)
    for k in ("id_c", "pos", "ori", "activ"):
        assert ora.gpu_vect_frags[k].tolist() == g["final_" + k], k


# ---- Appendix E ------------------------------------------------------------------------------------------------------------
def appendix_e_values(dev, state):
    per_pix = np.zeros(dev.n_pix)
    full = dev.evaluate(state, per_pix)
    n = len(state["pos"])
    pop, ids = O.new_state(n), np.zeros(n, np.int32)
    dev.pop_out(pop, state, ids, 1, 2)
    after_pix = np.zeros(dev.n_pix)
    after = dev.evaluate(pop, after_pix)
    delta = dev.sub_compute(pop, [0, 1, 2], [], np.arange(6, dtype=np.int32), per_pix)
    return (full, after, delta), (sum_bound(per_pix), sum_bound(after_pix), sum_bound(np.concatenate([per_pix, after_pix])))


def test_appendix_e_toy_values_of_the_host_recipe():
    """The values the reference's kernels give for the Appendix E toy through this recipe, recorded next to round 0's
    (which are 2.6e-8 away: DESIGN.md section 7).  The oracle is held to the recorded values everywhere, the library,
    where it exists, to the same."""
    t = APPENDIX_E["likelihood_toy"]
    want = (t["ref_host_full"], t["ref_host_full_after_eject_1"], t["ref_host_delta_kernel"])
    dev, state = toy_likelihood_problem()
    got, bounds = appendix_e_values(dev, state)
    for g, w, b in zip(got, want, bounds):
        assert abs(g - w) <= b, (g, w, b)
    for w, old in zip(want, (t["full"], t["full_after_eject_1"], t["delta_kernel"])):
        assert w == pytest.approx(old, rel=t["rel_tol"])
    if R.available():
        ref = R.RefKernels(dev.obs, dev.sub_id, dev.sub_len, dev.sub_accu, dev.dispatcher, dev.collector, dev.n_bins,
                           dev.nfpb, dev.param)
        got_r, _ = appendix_e_values(ref, state)
        assert got_r == want


# ---- the recorded fixtures -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("li", range(len(C.LAYOUTS)), ids=[lay["name"] for lay in C.LAYOUTS])
def test_oracle_and_frag_ops_reproduce_the_recorded_candidates(li):
    lay = C.LAYOUTS[li]
    out_f, wr_f, st_f = C.recorded_candidates(MUT, li)
    pairs = [(fA, fB) for fA, fBs in lay["proposals"] for fB in fBs]
    assert len(pairs) == len(out_f)
    refused = 0
    for i, (fA, fB) in enumerate(pairs):
        out_o, wr_o, st_o, _ = C.mutation_record(O.DenseOracle, lay, fA, fB)
        assert_candidates_equal((out_o, wr_o, st_o), (out_f[i], wr_f[i], st_f[i]), (lay["name"], fA, fB))
        refused += check_hostcheck_against(lay, fA, fB, out_f[i], wr_f[i], st_f[i])
    assert refused == len(C.OPS_NEEDING_FB) * sum(1 for fA, fB in pairs if fA == fB)


@pytest.mark.parametrize("li", range(len(C.LAYOUTS)), ids=[lay["name"] for lay in C.LAYOUTS])
def test_oracle_reproduces_the_recorded_likelihoods(li):
    lay = C.LAYOUTS[li]
    assert int(LIK["digest"][li]) == lay["digest"], "the regenerated inputs are not the recorded ones"
    dev = C.kernels_for(lay, O.DenseOracle)
    pix_f = LIK["l%d_pixels" % li]
    pix_o, tot_o = C.likelihood_record(dev, lay)
    assert np.array_equal(bits64(pix_o), bits64(pix_f))
    assert abs(tot_o - float(LIK["l%d_total" % li])) <= sum_bound(pix_f)
    deltas_f = LIK["l%d_deltas" % li]
    assert deltas_f.shape == (len(lay["proposals"]), C.K, C.N_OPS)
    for i, (fA, fBs) in enumerate(lay["proposals"]):
        d_o, bound = C.delta_record(dev, O.DenseOracle, lay, pix_f, fA, fBs)
        assert np.array_equal(np.isnan(d_o), np.isnan(deltas_f[i]))
        ok = ~np.isnan(d_o)
        assert np.all(np.abs(d_o - deltas_f[i])[ok] <= bound[ok]), (lay["name"], fA, fBs)


@pytest.mark.parametrize("li,params", RECORDED, ids=RECORDED_IDS)
def test_oracle_reproduces_the_recorded_likelihoods_under_parameter_sets(li, params):
    """ref_likelihood_params.npz holds no pixels: the oracle's own (bit-equal to the reference's where the library is, see
    test_full_evaluation_per_pixel_bit_equal) give the summation bounds."""
    lay = C.layout_under(li, params)
    param_cases.assert_not_default(lay["P"]["param_simu"])
    assert int(LIK_PARAMS[C.param_key(li, params, "digest")]) == lay["digest"], "the regenerated inputs are not the recorded ones"
    assert lay["digest"] != C.LAYOUTS[li]["digest"]
    dev = C.kernels_for(lay, O.DenseOracle)
    pix_o, tot_o = C.likelihood_record(dev, lay)
    total_f = float(LIK_PARAMS[C.param_key(li, params, "total")])
    param_cases.assert_reference_usable(total_f, (lay["name"], params))
    assert abs(tot_o - total_f) <= sum_bound(pix_o)
    deltas_f = LIK_PARAMS[C.param_key(li, params, "deltas")]
    assert deltas_f.shape == (len(lay["proposals"]), C.K, C.N_OPS)
    param_cases.assert_reference_usable(deltas_f[~np.isnan(deltas_f)], (lay["name"], params))
    for i, (fA, fBs) in enumerate(lay["proposals"]):
        d_o, bound = C.delta_record(dev, O.DenseOracle, lay, pix_o, fA, fBs)
        assert np.array_equal(np.isnan(d_o), np.isnan(deltas_f[i]))
        ok = ~np.isnan(d_o)
        assert np.all(np.abs(d_o - deltas_f[i])[ok] <= bound[ok]), (lay["name"], params, fA, fBs)


def test_recorded_parameter_sets_differ_from_the_recorded_defaults():
    """The sets move every recorded number: a kernel that ignored kuhn, lm, slope or d would reproduce ref_likelihood.npz instead."""
    for li in C.PARAM_LAYOUT_INDEX:
        totals = [float(LIK["l%d_total" % li])] + [float(LIK_PARAMS[C.param_key(li, n, "total")]) for n in param_cases.NAMES]
        assert len(set(totals)) == len(totals), totals
        for a, b in zip(totals, totals[1:]):
            assert abs(a - b) > 1e-6 * abs(a)


@needs_ref
def test_regenerating_the_fixtures_gives_identical_arrays():
    mut, lik = C.fixture_arrays(R.RefKernels)
    par = C.param_fixture_arrays(R.RefKernels)
    for name, new, old in (("ref_mutations", mut, MUT), ("ref_likelihood", lik, LIK), ("ref_likelihood_params", par, LIK_PARAMS)):
        assert sorted(new) == sorted(old.files), name
        for k in new:
            a, b = np.asarray(new[k]), old[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, k)
