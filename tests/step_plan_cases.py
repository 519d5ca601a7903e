"""Shared by tests/test_step_plan_gpu.py and its child process: one small case per flow a candidate evaluation can take
(graal_amd/csrc/step_plan.h) -- a problem, a layout built for the flow, two proposals.  ``run_case`` evaluates the proposals on a fresh
engine and returns the candidates' scores, the moves of graal_run_counters and the facts the plan read.  One rank: graal_eval_candidates,
whose float64 scores are a fixed function of the int64 Q and coarse sums (graal_eval_candidates_x serves only a handle with an exchange of two
ranks and more attached); they are compared as 64-bit words.  ``python -m tests.step_plan_cases out.npz`` stores the scores of every case (the child runs it with GRAAL_STRICT_DENSE=1 in its environment:
the O(m^2) validation kernel instead of the windowed reference-arithmetic kernels).  A second argument chooses the cases ("strict", or their
positions in CASES: "0,8"), a third puts parameter sets of tests/param_cases.py behind them ("fitted_a,fitted_b": scores stored as d<i>_<set>;
tests/test_model_params_gpu.py)."""
import sys

import numpy as np

from graal_amd import synth
from tests import strict_cases

_cache = {}


def _cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def _mid():      # one sub-fragment per bin, a window of ~60 bins (the problem of strict_cases' K = 10 case, smaller)
    return _cached("mid", lambda: strict_cases._problem(n_bins=1000, nnz=40000, seed=21, n_sub=1, weights=(5, 3, 2), mean_len_bp=660.0, accu=1,
                                                        fact=1e4, v_inter=1e-3, d_max=40.0))


def _late():     # three sub-fragments per bin, one RF count: tiles of 32
    return _cached("late", lambda: strict_cases._problem(n_bins=520, nnz=25000, seed=22, n_sub=3, weights=(5, 3, 2), mean_len_bp=700.0, accu=9,
                                                         d_max=40.0))


def _long():     # exact arithmetic against the dense oracle: coordinates on a grid, the window the whole contig
    return _cached("long", lambda: synth.with_dense(synth.make_problem(
        n_bins=1300, nnz=40000, n_sub=1, seed=23, contig_weights=(5, 3, 2), mean_len_bp=1500.0, accu=1,
        param=synth.make_param_simu(fact=1.0e4, v_inter=1.0e-3), grid_bp=2000)))


def _many():     # many contacts in short rows: the indexed producer's ground
    return _cached("many", lambda: strict_cases._problem(n_bins=1500, nnz=150000, seed=24, n_sub=1, weights=(5, 3, 2), mean_len_bp=660.0, accu=1,
                                                         fact=1e4, v_inter=1e-3, d_max=40.0))


def _rep():
    from tests.test_strict_windowed_gpu import rep_problem_ref
    return _cached("rep", lambda: rep_problem_ref(3, 181))


def _r(a, b):
    return np.arange(a, b)


# name -> problem, the contigs the layout must hold (the rest: contigs of 1 .. rest_max fragments), arithmetic, two proposals, layout seed, scan path
CASES = {
    "contigs of at most 16": dict(problem=_mid, groups=[], rest_max=12, strict=True, props=[(10, [120, 310, 500]), (700, [5, 350, 999])]),
    "contigs of about 40": dict(problem=_mid, groups=[_r(0, 40), _r(100, 141), _r(300, 338)], rest_max=12, strict=True,
                                props=[(10, [120, 310, 500]), (130, [5, 35, 320])]),
    "contigs of 65 to 256": dict(problem=_mid, groups=[_r(0, 200), _r(200, 300), _r(400, 550)], rest_max=12, strict=True,
                                 props=[(50, [150, 250, 500]), (420, [10, 299, 700])]),
    "contigs of 257 and more": dict(problem=_mid, groups=[_r(0, 400), _r(400, 700)], rest_max=12, strict=True,
                                    props=[(100, [300, 450, 800]), (650, [0, 399, 401])]),
    "late stage: two contigs of 260": dict(problem=_late, groups=[_r(0, 260), _r(260, 520)], rest_max=12, strict=True,
                                           props=[(100, [101, 300, 519]), (400, [0, 259, 261])]),
    "exact arithmetic, a contig of 1,100": dict(problem=_long, groups=[_r(0, 1100)], rest_max=12, strict=False,
                                                props=[(500, [501, 1200]), (1250, [3, 1099])]),
    "short rows: the indexed producer": dict(problem=_many, groups=[], rest_max=4, strict=True, props=[(10, [700, 1400]), (800, [3, 1200])], seed=7),
    "short rows, forced to stream": dict(problem=_many, groups=[], rest_max=4, strict=True, props=[(10, [700, 1400]), (800, [3, 1200])], seed=7, scan_path=1),
    "repeated bins": dict(problem=_rep, repeats=True, strict=True, props=[(7, [3, 20, 41]), (40, [7, 12, 30])]),
}
STRICT = [name for name, c in CASES.items() if c["strict"]]


def layout_of(name, params=None):
    """(problem, layout, max_id) of a case; the layout is the same whoever builds it.  params: a parameter set of tests/param_cases.py put
    behind the problem (contacts and layout untouched); None: the case's own parameters."""
    from tests.test_engine_gpu import relabel_ref
    from tests.test_scan_rows_gpu import layout_of_groups
    c = CASES[name]
    P = c["problem"]()
    if params is not None:
        from tests import param_cases
        P = param_cases.with_params(P, params)
    rng = np.random.RandomState(c.get("seed", len(name)))
    if c.get("repeats"):
        from tests.test_repeats_gpu import random_state_with_repeats
        s = random_state_with_repeats(P, rng, n_contigs=9)
    else:
        s = layout_of_groups(P, rng, list(c["groups"]), rest_max=c["rest_max"])
    return P, s, relabel_ref(s)


def run_case(name, params=None):
    from tests.test_repeats_gpu import engine_with_repeats, split_observations
    from tests.test_scan_rows_gpu import engine_for
    c = CASES[name]
    P, s, max_id = layout_of(name, params)
    e = engine_with_repeats(P, s) if c.get("repeats") else engine_for(P, s)
    row = split_observations(P)[0][0] if c.get("repeats") else P["coo_row"]
    e.set_mode(ref_trans_accu=c["strict"], strict=c["strict"])
    assert e.relabel_contigs() == max_id
    e.set_scan_path(c.get("scan_path", 0))
    before = e.run_counters()
    deltas = [np.array(e.eval_candidates(fA, np.asarray(fBs, np.int32), max_id), np.float64) for fA, fBs in c["props"]]
    after = e.run_counters()
    e.close()
    n_sub = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)[:, 3]
    return dict(deltas=np.stack(deltas), moved={k: after[k] - before[k] for k in after}, counters=after,
                # what the plan read (step_plan.h: StepFacts), from the inputs alone
                facts=dict(n=len(s["id_c"]), n_sub_total=int(P["init_n_sub_frags"]), nnz=len(row), single_sub=int(n_sub.max() == 1),
                           n_contigs=max_id + 1, max_lcont=int(s["l_cont"].max()), lcont_bound=int(s["l_cont"].max()),
                           has_rep=int(bool(c.get("repeats"))), strict=int(c["strict"]), quirk=int(c["strict"]), K=len(c["props"][0][1]),
                           has_rowptr=int(np.all(np.diff(row) >= 0)), longest_row=int(np.bincount(row).max()),
                           forced_producer=c.get("scan_path", 0)))


if __name__ == "__main__":
    which = sys.argv[2] if len(sys.argv) > 2 else ""
    if which and all(x.isdigit() for x in which.split(",")):             # (positions in CASES: "0,8")
        names = [list(CASES)[int(x)] for x in which.split(",")]
    else:
        names = STRICT if which == "strict" else list(CASES)
    params =sys.argv[3].split(",") if len(sys.argv) > 3 else [None]      # (parameter sets of tests/param_cases.py: keys d<i>_<set>)
    out = {}
    for i, name in enumerate(CASES):
        if name in names:
            for p in params:
                out["d%d" % i + ("_" + p if p else "")] = run_case(name, p)["deltas"]
    np.savez(sys.argv[1], **out)
