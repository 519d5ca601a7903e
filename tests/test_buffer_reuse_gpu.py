"""One handle taken through problems whose n, S and nnz all go up and down must answer every call that owns buffers exactly as a fresh
handle given the same problem does: the per-layout sets (reallocated when n or S changes), the grow-only arrays (used below their
allocation after a larger problem) and the core's own buffers may carry nothing of the handle's history into any word of any output.
Nothing here is compared with stored numbers: the other GPU tests tie a fresh handle's results to the restatements.

The problems are junction_reference's: "sub1" (120 bins x 1), "sub3" (48 bins x 3), the circular case (45 bins x 3), "sub1" again.  The
second test drives the grow-only arrays inside one problem: the span arrays (3 spans, the full tiling, 3 again) and the windows' images
and origins (1 window, 8, 1 again)."""
import numpy as np
import pytest

from graal_amd import flips, swaps
from graal_amd.lib import Engine
from tests import junction_reference as JR
from tests.engine_states import cached

pytestmark = pytest.mark.gpu

SEQUENCE = ("sub1", "sub3", "circ", "sub1")
F_A, F_BS = 7, (8, 30, 40)                      # one fixed proposal, K = 3 (every problem has at least 45 fragments)
WINDOWS = ((0, 0), (5, 20))
SEED = 20240229


def problem(name):
    return cached(("buffer_reuse", name), lambda: JR.case(name))


def upload(e, P):
    """engine_states.engine_for's order, on a handle that may have served another problem."""
    e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                      P["mean_squared_frags_per_bin"])
    e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
    e.set_params(P["param_simu"])
    e.upload_frags(P["S_o_A_frags"])


def flat(x):
    if isinstance(x, dict):
        x = tuple(x[k] for k in sorted(x))
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in flat(y)]
    return [np.asarray(x)]


def first_tiling(mod, s):
    return next(iter(mod.tilings(s)))


def every_call(e):
    """Every call that owns buffers, in one fixed order; the calls that rewrite the layout last.  {name: flat list of arrays}."""
    out = {}
    stats, max_id = e.begin_step()                     # (the relabel a full evaluation asks for after an upload)
    out["begin"] = (stats, max_id)
    out["full"] = e.eval_full_q().astype(np.int64)
    out["candidates"] = e.eval_candidates(F_A, list(F_BS), max_id)
    s = e.download_frags()
    out["layout"] = s
    out["junctions"] = e.junction_scores_q()
    out["rings"] = e.ring_scores_q()
    out["links"] = e.end_links_q()
    out["best"] = e.end_links_best()
    out["insertions"] = e.insertions_q()
    fl, sw = first_tiling(flips, s), first_tiling(swaps, s)
    out["flips"] = e.block_flips_q(*fl)
    out["swaps"] = e.block_swaps_q(*sw)
    out["excisions"] = e.block_excisions_q(*fl)
    out["maps"] = e.layout_maps(max_px=64)
    out["windows"] = e.map_windows(WINDOWS, 16, 16, bin=1)
    out["simulated"] = e.simulate_contacts(SEED)
    # one cut and its re-join in one edit, then one linear contig closed into a ring
    linear = (s["circ"] == 0) & (s["next"] != -1)
    f = int(np.nonzero(linear)[0][0])
    out["edit"] = e.edit_layout(cuts=[f], joins=[(2 * f + 1, 2 * int(s["next"][f]))])
    s = e.download_frags()
    out["edited"] = s
    ring = int(np.nonzero((s["circ"] == 0) & (s["l_cont"] >= 2))[0][0])
    out["close"] = e.close_rings([ring])
    out["begin_closed"] = e.begin_step()
    out["closed"] = e.download_frags()
    out["full_closed"] = e.eval_full_q().astype(np.int64)
    return {k: flat(v) for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def same(got, want, where):
    assert len(got) == len(want), where
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (where, i)
        assert np.array_equal(bits(g), bits(w)), (where, i)       # (word by word: a NaN pixel equals itself)


def on_fresh(P, fn):
    e = Engine(0)
    try:
        upload(e, P)
        return fn(e)
    finally:
        e.close()


def test_reused_handle_equals_fresh_handle_across_problems():
    shapes = [(P["n_frags"], P["init_n_sub_frags"], len(P["coo_row"])) for P in map(problem, SEQUENCE)]
    for k in range(3):                                   # n, S and nnz each go down and up along the sequence
        d = np.sign(np.diff([x[k] for x in shapes]))
        assert -1 in d and 1 in d, (k, shapes)
    e = Engine(0)
    try:
        for step, name in enumerate(SEQUENCE):
            P = problem(name)
            upload(e, P)
            got = every_call(e)
            want = cached(("buffer_reuse_fresh", name), lambda: on_fresh(P, every_call))
            assert got.keys() == want.keys()
            for call in got:
                same(got[call], want[call], (step, name, call))
    finally:
        e.close()


def test_grow_only_arrays_serve_smaller_calls():
    P = problem("sub1")
    fl = max(flips.tilings(P["S_o_A_frags"]), key=lambda x: len(x[0]))
    assert len(fl[0]) > 3
    few = tuple(a[:3] for a in fl)
    origins = [(3 * k, 5 * k) for k in range(8)]
    calls = [("flips3", lambda e: e.block_flips_q(*few)), ("flips_all", lambda e: e.block_flips_q(*fl)),
             ("flips3", lambda e: e.block_flips_q(*few)),
             ("win1", lambda e: e.map_windows(origins[:1], 16, 16, bin=1)), ("win8", lambda e: e.map_windows(origins, 16, 16, bin=1)),
             ("win1", lambda e: e.map_windows(origins[:1], 16, 16, bin=1))]
    e = Engine(0)
    try:
        upload(e, P)
        for step, (name, fn) in enumerate(calls):
            got = flat(fn(e))
            want = cached(("buffer_reuse_grow", name), lambda: flat(on_fresh(P, fn)))
            same(got, want, (step, name))
    finally:
        e.close()
