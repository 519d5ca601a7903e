"""graal_simulate_contacts on a layout with dense rows: every branch of the row sorter (k_sim_place: rank in one pass up to 256 entries,
bitonic network up to 4096, tiled ranks above, a second tile above 8192), the zero-truncated Poisson's rejection loop (background
lambda >= 10) and thinning under heavy rejection (Lmax / lambda_b = 25000), each compared entry by entry and in order with the numpy
restatement restricted to chosen rows (tests/sim_reference.py, rows=).

The "hubs" layout: tests/test_simulate_gpu.py's "chunks" layout (9000 bins of one sub-fragment in three contigs, v_inter 2e-4) with RF
count 1 everywhere (n_frags_per_bins = 1.0) except a few hub sub-fragments, whose RF counts make their own rows dense: lambda_b =
v_inter * accu_hub * accu_b.  The conditions this layout must meet (row lengths, no flagged draw in a hub row) are asserted without a GPU
in tests/test_simulate_cpu.py."""
import math
import time

import numpy as np
import pytest

from graal_amd import synth
from graal_amd.lib import Engine
from tests import sim_reference as R

pytestmark = pytest.mark.gpu

SEED = 77
# hub sub-fragment id -> RF count, and the length of its row in the reference at SEED.  How they were found: on the CPU, once, with
# R.simulate(rows=[id]).  The two 25000 hubs (a two-tile row and the largest background lambda, 125000 between them) and 40 / 90 / 150
# (round RF counts, any length inside a branch) were set first.  The four rows of an exact length were then tuned FROM THE HIGHEST ID
# DOWN, because a row's length depends on the RF counts of all higher ids (an accepted candidate consumes draws and shifts the rest of
# its chunk's stream) and on no lower one: for each, walk the id upwards from a start and nudge the RF count by (target - length) / 1.7
# (a row gains about 1.7 entries per RF count here) until the length is the target.  A change to any RF count, to the layout or to
# SEED needs the ids below it tuned again; test_simulate_cpu.py::test_hubs_layout_reaches_every_branch says so when it does.
HUBS = {
    4000: (25000, 4961),    # one tile
    1206: (3591, 4096),     # the full, unpadded network
    759: (3356, 4097),      # first row of the tile branch
    338: (135, 256),        # last row of the one-pass branch
    243: (121, 257),        # first row of the network, padded to 512
    150: (200, 424),        # network, padded to 512
    90: (1000, 1681),       # network, padded to 2048
    40: (5000, 5811),       # one tile
    3: (25000, 8952),       # two tiles
}
# ordinary rows (RF count 1: Lmax = 5 against lambda_b = 2e-4, almost every candidate rejected), spread over the three contigs and the
# three chunks, and the rows before and after each chunk edge
ORDINARY = (0, 1, 500, 2500, 3999, 4001, 6000, 8990, R.CHUNK - 1, R.CHUNK, 2 * R.CHUNK - 1, 2 * R.CHUNK)
ROWS = tuple(sorted(set(HUBS) | set(ORDINARY)))

_cache = {}


def hubs_problem():
    if "problem" not in _cache:
        par = synth.make_param_simu(fact=30.0, v_inter=2e-4)
        P = synth.make_problem(n_bins=9000, nnz=500, n_sub=1, seed=31, contig_weights=(4, 3, 3), accu=1, param=par)
        P["S_o_A_frags"] = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
        P["S_o_A_frags"]["ori"][::5] = -1
        ids, acc = np.asarray(P["np_sub_frags_id"]), np.array(P["np_sub_frags_accu"])
        assert np.array_equal(ids[:, 0], np.arange(len(ids))) and P["mean_squared_frags_per_bin"] == 1.0
        for h, (a, _) in HUBS.items():
            acc[h, 0] = a                       # (n_sub 1: sub-fragment id = bin, slot 0)
        P["np_sub_frags_accu"] = acc
        _cache["problem"] = (P, par)
    return _cache["problem"]


def hubs_reference():
    """(row, col, count, flagged pairs, flagged chunks) of ROWS, built once and shared; callers leave it unchanged."""
    if "reference" not in _cache:
        P, par = hubs_problem()
        t0 = time.perf_counter()
        want = R.simulate(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"], par,
                          P["S_o_A_frags"], SEED, rows=ROWS)
        print("hubs reference: %d rows, %d entries, %d + %d flagged draws, %.2f s"
              % (len(ROWS), len(want[0]), len(want[3]), len(want[4]), time.perf_counter() - t0))
        for x in want[:3]:
            x.setflags(write=False)
        _cache["reference"] = want
    return _cache["reference"]


def reference_row(a):
    r, c, v = hubs_reference()[:3]
    m = r == a
    return c[m], v[m]


def _gpu_lists():
    """The GPU's list of the layout, twice from one engine (the second call reuses the first one's buffers); prints the call's time."""
    if "gpu" not in _cache:
        P, par = hubs_problem()
        e = Engine(0)
        try:
            e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                              P["mean_squared_frags_per_bin"])
            e.set_params(par)
            e.upload_frags(P["S_o_A_frags"])
            # (Engine.simulate_contacts raises unless graal_simulate_contacts returned GRAAL_OK, which it does only with none of the
            # kernels' disagreement flags set)
            first = e.simulate_contacts(SEED)
            t0 = time.perf_counter()
            second = e.simulate_contacts(SEED)
            dt = time.perf_counter() - t0
        finally:
            e.close()
        print("hubs simulation: %d contacts, %.1f ms per call incl. the copy to the host" % (len(first[0]), 1e3 * dt))
        _cache["gpu"] = (first, second)
    return _cache["gpu"]


def _gpu_row(got, a):
    r, c, v = got
    lo, hi = np.searchsorted(r, a, "left"), np.searchsorted(r, a, "right")
    return c[lo:hi], v[lo:hi]


@pytest.mark.parametrize("hub", sorted(HUBS))
def test_hub_row_equals_reference_in_order(hub):
    """Exact: no draw of a hub row is flagged (asserted on the CPU), so nothing excuses a difference."""
    want = hubs_reference()
    assert not any(p[0] == hub for p in want[3]) and not any(k[0] == hub for k in want[4])
    wc, wv = reference_row(hub)
    gc, gv = _gpu_row(_gpu_lists()[0], hub)
    assert len(wc) == HUBS[hub][1]
    assert len(gc) == len(wc), (hub, len(gc), len(wc))
    bad = np.nonzero((gc != wc) | (gv != wv))[0]
    assert len(bad) == 0, (hub, len(bad), bad[:5], gc[bad[:5]], wc[bad[:5]], gv[bad[:5]], wv[bad[:5]])


def test_ordinary_rows_equal_reference():
    """tests/test_simulate_gpu.py's rule over the ordinary rows; and where nothing differs, the order too."""
    want = hubs_reference()
    got = _gpu_lists()[0]
    m = np.isin(got[0], ORDINARY)
    w = np.isin(want[0], ORDINARY)
    diff, unexplained = R.compare(tuple(x[m] for x in got), tuple(x[w] for x in want[:3]), want[3], want[4])
    n = int(w.sum())
    assert n > 20
    assert unexplained == [], unexplained[:10]
    assert len(diff) <= math.ceil(1e-4 * n), (len(diff), n)
    if not diff:
        assert all(np.array_equal(x[m], y[w]) for x, y in zip(got, want[:3]))


def test_whole_list_well_formed_and_repeatable():
    from tests.test_simulate_gpu import _well_formed
    P, par = hubs_problem()
    first, second = _gpu_lists()
    S = P["init_n_sub_frags"]
    _well_formed(*first, S)
    assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(first, second))
    # every hub column, in the reference rows above it: the same entry or none on both sides (outside flagged draws)
    want = hubs_reference()
    g = {(int(r), int(c)): int(v) for r, c, v in zip(*(x[np.isin(first[1], list(HUBS)) & np.isin(first[0], ROWS)] for x in first))}
    w = {(int(r), int(c)): int(v) for r, c, v in zip(*(x[np.isin(want[1], list(HUBS))] for x in want[:3]))}
    seen = 0
    for h in HUBS:
        for a in ROWS:
            if a >= h or (a, h) in want[3] or (a, h // R.CHUNK) in want[4]:
                continue
            assert g.get((a, h)) == w.get((a, h)), (a, h, g.get((a, h)), w.get((a, h)))
            seen += (a, h) in w
    assert seen > 30
    # the hub rows hold most of the list; the ordinary rows' background lands in hub columns
    assert len(first[0]) > sum(n for _, n in HUBS.values())
