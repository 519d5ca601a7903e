"""The mid-size cases of the indexed contact producer (k_scan_rows): seeded problems from synth.make_problem, layouts with contigs of
exact lengths, and the evaluations to run on them.  Each case is NAMED for the part of the kernel it is built to reach, carries the
`flaw` of tests/scan_rows_reference.py that it must expose, and has a check -- `engages` -- that it does reach that part; the CPU suite
runs the checks (tests/test_scan_rows_reference_cpu.py), the GPU tests run them again before they launch anything
(tests/test_scan_rows_midsize_gpu.py), so that a change of seed cannot quietly empty a test.

Nothing here needs a device."""
import functools

import numpy as np

from graal_amd import synth
from tests import scan_rows_reference as R
from tests.test_scan_rows_gpu import layout_of_groups, numpy_count

ROW_LENGTHS = (0, 1, 64, 65, 511, 512, 513, 1024, 1025)     # around the 64 lanes, the 512 contacts of a trip and two trips
ROW_LENGTHS_SUB3 = (0, 1, 65, 512, 513, 1025)


@functools.lru_cache(maxsize=None)
def _problem(n_sub, n_bins, nnz, seed):
    par = synth.make_param_simu(fact=300.0, v_inter=0.03)
    accu = 1 if n_sub == 1 else ("random", 3, 12)
    return synth.make_problem(n_bins=n_bins, nnz=nnz, n_sub=n_sub, seed=seed, contig_weights=(5, 3, 2), mean_len_bp=1500.0, accu=accu, param=par)


def base_problem(n_sub):
    """About 2,600 bins of one sub-fragment, or about 900 bins of three with mixed RF counts."""
    return _problem(1, 2600, 150_000, 81) if n_sub == 1 else _problem(3, 900, 150_000, 82)


def with_contacts(P, row, col, val):
    """P with another (row, col)-sorted, duplicate-free contact list -- and the bin-level map that goes with it."""
    row, col, val = np.asarray(row, np.int32), np.asarray(col, np.int32), np.asarray(val, np.int32)
    S = int(P["init_n_sub_frags"])
    keys = row.astype(np.int64) * S + col
    assert np.all(row < col) and np.all(keys[1:] > keys[:-1]), "sorted by (row, col), no duplicates, row < col"
    P = dict(P, coo_row=row, coo_col=col, coo_val=val)
    n_bins, b = P["n_frags"], P["bin_of_sub"]
    bi, bj = b[row].astype(np.int64), b[col].astype(np.int64)
    m = bi != bj
    ub, inv = np.unique(np.minimum(bi[m], bj[m]) * n_bins + np.maximum(bi[m], bj[m]), return_inverse=True)
    P["bin_coo_row"], P["bin_coo_col"] = (ub // n_bins).astype(np.int32), (ub % n_bins).astype(np.int32)
    P["bin_coo_val"] = np.bincount(inv, weights=val[m].astype(np.float64)).astype(np.float32)
    return P


def with_row_lengths(P, rows, lengths, rng):
    """The chosen rows trimmed (a random subset kept) or padded (new distinct cols > row, count 1) to exactly `lengths` contacts."""
    S = int(P["init_n_sub_frags"])
    row, col, val = P["coo_row"], P["coo_col"], P["coo_val"]
    keep = np.ones(len(row), bool)
    add_r, add_c = [], []
    for r, L in zip(rows, lengths):
        r, L = int(r), int(L)
        assert S - 1 - r >= L, "row %d cannot hold %d contacts" % (r, L)
        mine = np.flatnonzero(row == r)
        if len(mine) > L:
            keep[rng.choice(mine, len(mine) - L, replace=False)] = False
        elif len(mine) < L:
            free = np.setdiff1d(np.arange(r + 1, S), col[mine])
            new = rng.choice(free, L - len(mine), replace=False)
            add_r.append(np.full(len(new), r))
            add_c.append(new)
    row, col, val = row[keep], col[keep], val[keep]
    if add_r:
        row = np.concatenate([row] + add_r)
        col = np.concatenate([col] + add_c)
        val = np.concatenate([val, np.ones(len(row) - len(val), val.dtype)])
        o = np.argsort(row.astype(np.int64) * S + col, kind="stable")
        row, col, val = row[o], col[o], val[o]
    P = with_contacts(P, row, col, val)
    for r, L in zip(rows, lengths):
        assert np.count_nonzero(P["coo_row"] == r) == L
    return P


def _fill(rng, first, size, taken, n):
    """`first` (deduplicated, in order, without what is taken) topped up with random fragments to `size`; marks them taken."""
    out = []
    for f in first:
        if not taken[f] and len(out) < size:
            taken[f] = True
            out.append(int(f))
    free = rng.permutation(np.flatnonzero(~taken))[:size - len(out)]
    taken[free] = True
    out = np.concatenate([np.asarray(out, np.int64), free])
    assert len(out) == size
    return rng.permutation(out)


def _refs(case, flaw=None):
    P, s = case["P"], case["state"]
    return [R.indexed_pass(P["coo_row"], P["coo_col"], P["bin_of_sub"], s["id_c"], fA, fBs, int(s["l_cont"].max()), flaw=flaw, flaw_arg=case.get("flaw_arg"))
            for fA, fBs in case["evals"]]


def references(case):
    return _refs(case)


def flawed_references(case):
    return _refs(case, case["flaw"])


# ---- exact row lengths ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_row_lengths(n_sub):
    """Rows of exactly 0 .. 1,025 contacts inside two contigs of a few hundred fragments: the clamped load, the ballots and the slot offsets at
    the lanes' and the trips' edges; the second and the third trip of the c0 loop.  K = 1 and K = 3."""
    P0 = base_problem(n_sub)
    rng = np.random.RandomState(810 + n_sub)
    S, n, b = int(P0["init_n_sub_frags"]), P0["n_frags"], P0["bin_of_sub"]
    lengths = ROW_LENGTHS if n_sub == 1 else ROW_LENGTHS_SUB3
    cand = np.arange(40, S - 1100)
    if n_sub == 3:
        cand = cand[b[cand] != b[cand - 1]]                      # first sub-fragments of their bins: no two chosen rows share a bin
    rows = np.sort(rng.choice(cand, len(lengths), replace=False))
    P = with_row_lengths(P0, rows, lengths, rng)
    size = (310, 330) if n_sub == 1 else (150, 160)
    first = ([], [])
    for i, r in enumerate(rows):    # the row's bin; its first and last col, the first col of every later trip, and a few more: all in the two contigs
        cols = P["coo_col"][P["coo_row"] == r]
        pick = [r] + [cols[j] for j in (0, 64, 511, 512, 1023, 1024, len(cols) - 1) if 0 <= j < len(cols)]
        pick += list(rng.choice(cols, min(len(cols), 6), replace=False)) if len(cols) else []
        first[i % 2].extend(int(b[x]) for x in pick)
    own = [[int(b[r]) for r in rows[k::2]] for k in (0, 1)]      # the rows' own bins: alternately in the first and the second contig
    taken = np.zeros(n, bool)
    taken[own[1]] = True                                         # (not to be claimed by the first contig as some row's col)
    groups = [_fill(rng, own[0] + first[0], size[0], taken, n)]
    taken[own[1]] = False
    groups.append(_fill(rng, own[1] + first[1], size[1], taken, n))
    s = layout_of_groups(P, rng, groups)
    small = int(np.flatnonzero(s["l_cont"] <= 12)[0])
    evals = [(own[0][0], np.asarray([own[1][0]], np.int32)),
             (own[1][-1], np.sort(np.asarray([own[0][-1], int(groups[1][0]) if int(groups[1][0]) != own[1][-1] else int(groups[1][1]), small], np.int32)))]
    return dict(name="exact_row_lengths", P=P, state=s, evals=evals, rows=rows, lengths=lengths, flaw="first_trip_only", also_flaws=("short_slice",))


def engages_exact_row_lengths(case, refs):
    for ref in refs:
        at = np.searchsorted(ref["ids"], case["rows"])
        assert np.array_equal(ref["ids"][at], case["rows"]), "a chosen row is not affected"
        got = ref["hi"][at] - ref["lo"][at]
        assert list(got) == list(case["lengths"])
        assert np.all(ref["per_row"][at][got > 0] >= 1), "a chosen row queues nothing"
        assert ref["shape"]["rows_over_512"] >= 2 and ref["shape"]["rows_over_1024"] >= 1          # second and third trips of the c0 loop
        assert ref["shape"]["bound"] <= R.ROWS_CAP and ref["count"] >= 1
        # the last contact of every chosen row -- the one a slice of hi - 1 loses, the 513th, the 1,025th -- is queued
        P = case["P"]
        mark = np.zeros(len(P["bin_of_sub"]), bool)
        mark[ref["ids"]] = True
        for a, n_c in zip(at, got):
            if n_c:
                assert mark[P["coo_col"][ref["hi"][a] - 1]]
    assert sorted(len(fBs) for _, fBs in case["evals"]) == [1, 3]


# ---- at the cap -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def at_the_cap(n_sub, over=False):
    """K = 1, fA and its neighbour in two contigs whose rows fill the kernel's list: 2 x 1,024 fragments of one sub-fragment (2,048 rows, every
    wave makes 8 trips), 2 x 341 bins of three (bound 2,046).  over: the first contig one longer -- the host must refuse the indexed pass."""
    P = base_problem(n_sub)
    rng = np.random.RandomState(820 + n_sub)
    n = P["n_frags"]
    L = 1024 if n_sub == 1 else 341
    taken = np.zeros(n, bool)
    groups = [_fill(rng, [], L + (1 if over else 0), taken, n), _fill(rng, [], L, taken, n)]
    flaw_arg = None
    if n_sub == 1 and not over:
        # the last listed row can queue nothing (row < col), so the last row that CAN matter is the one before it: give it a contact
        ids = np.sort(np.concatenate(groups))
        a, c = int(ids[-2]), int(ids[-1])
        row, col, val = P["coo_row"], P["coo_col"], P["coo_val"]
        if not np.any((row == a) & (col == c)):
            at = int(np.searchsorted(row.astype(np.int64) * int(P["init_n_sub_frags"]) + col, a * int(P["init_n_sub_frags"]) + c))
            P = with_contacts(P, np.insert(row, at, a), np.insert(col, at, c), np.insert(val, at, 1))
        flaw_arg = R.ROWS_CAP - 2
    s = layout_of_groups(P, rng, groups)
    evals = [(int(groups[0][0]), np.asarray([int(groups[1][0])], np.int32))]
    return dict(name="at_the_cap", P=P, state=s, evals=evals, over=over, flaw="drop_listed_from" if flaw_arg else "first_row_per_wave_only", flaw_arg=flaw_arg)


def engages_at_the_cap(case, refs):
    (ref,) = refs
    sh, single = ref["shape"], len(case["P"]["bin_of_sub"]) == case["P"]["n_frags"]
    if case["over"]:
        assert sh["bound"] == (2050 if single else 2052) and sh["bound"] > R.ROWS_CAP
        return
    assert sh["bound"] == (2048 if single else 2046) and sh["bound"] <= R.ROWS_CAP and sh["n_rows"] <= R.ROWS_CAP
    assert sh["grid"] == 64 and ref["count"] >= 1
    if single:
        assert sh["n_rows"] == R.ROWS_CAP and sh["trips_per_wave"] == 8                 # the list is full
        assert ref["per_row"][R.ROWS_CAP - 2] >= 1
    else:
        assert 2000 <= sh["n_rows"] <= 2046 and sh["trips_per_wave"] == 8


# ---- the round robin over rows ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def round_robin(n_sub):
    """K = 5 with contigs of 60-120 fragments: more rows than the grid's 256 waves, a list far from full."""
    P = base_problem(n_sub)
    rng = np.random.RandomState(830 + n_sub)
    n = P["n_frags"]
    sizes = (60, 75, 90, 100, 110, 120) if n_sub == 1 else (60, 70, 80, 90, 100, 110)
    taken = np.zeros(n, bool)
    groups = [_fill(rng, [], k, taken, n) for k in sizes]
    s = layout_of_groups(P, rng, groups)
    evals = [(int(groups[0][0]), np.sort(np.asarray([int(g[0]) for g in groups[1:]], np.int32))),
             (int(groups[5][3]), np.sort(np.asarray([int(g[1]) for g in groups[:5]], np.int32)))]
    return dict(name="round_robin", P=P, state=s, evals=evals, flaw="first_row_per_wave_only")


def engages_round_robin(case, refs):
    for ref in refs:
        sh = ref["shape"]
        assert 256 < sh["bound"] <= R.ROWS_CAP and sh["grid"] == 64 and sh["n_waves"] == 256
        assert sh["n_rows"] > 256 and sh["trips_per_wave"] >= 2 and sh["n_rows"] < R.ROWS_CAP - 256
        assert ref["per_row"][256:].sum() >= 1 and ref["count"] >= 1


# ---- more bitmap words than threads -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_words(n_sub):
    """More than 8,192 ids: a thread lists several words of the bitmap.  Affected ids in the first, a middle and the last word, the very last id
    among them; contigs of tens of fragments."""
    P = _problem(1, 9001, 200_000, 84) if n_sub == 1 else _problem(3, 3000, 200_000, 85)
    rng = np.random.RandomState(840 + n_sub)
    S, n, b = int(P["init_n_sub_frags"]), P["n_frags"], P["bin_of_sub"]
    row, col = P["coo_row"], P["coo_col"]
    last = S - 1
    to_last = np.flatnonzero(col == last)
    high = np.flatnonzero(row >= 32 * R.ROWS_THREADS)            # rows a listing of one word per thread never reaches
    assert len(to_last) and len(high)
    c_last, c_high = int(to_last[0]), int(high[len(high) // 2])
    low = np.flatnonzero((row < 32) & (col > 32))
    mid = np.flatnonzero((row // 32 == (S // 2) // 32))
    first0 = [b[row[low[0]]], b[col[low[0]]], b[last], b[row[c_last]], b[row[c_high]], b[col[c_high]]]
    first1 = [b[row[mid[0]]], b[col[mid[0]]]]
    taken = np.zeros(n, bool)
    groups = [_fill(rng, first0, 30, taken, n), _fill(rng, first1, 40, taken, n), _fill(rng, [], 25, taken, n)]
    s = layout_of_groups(P, rng, groups)
    evals = [(int(b[last]), np.sort(np.asarray([int(groups[1][0]), int(groups[2][0])], np.int32))),
             (int(groups[1][1]), np.sort(np.asarray([int(groups[0][2])], np.int32)))]
    return dict(name="many_words", P=P, state=s, evals=evals, flaw="one_word_per_thread")


def engages_many_words(case, refs):
    S = int(case["P"]["init_n_sub_frags"])
    assert S >= 8990 and (len(case["P"]["bin_of_sub"]) != case["P"]["n_frags"] or S % 32 != 0)
    for ref in refs:
        sh, ids = ref["shape"], ref["ids"]
        assert sh["words_per_thread"] >= 2 and sh["bound"] <= R.ROWS_CAP
        words = ids // 32
        assert words.min() == 0 and words.max() == (S - 1) // 32 and ids.max() == S - 1
        assert np.any((words > 64) & (words < 200))
        assert ref["per_row"][ids >= 32 * R.ROWS_THREADS].sum() >= 1 and ref["count"] >= 1


CASES = {
    "exact_row_lengths-1": (exact_row_lengths, (1,), engages_exact_row_lengths),
    "exact_row_lengths-3": (exact_row_lengths, (3,), engages_exact_row_lengths),
    "at_the_cap-1": (at_the_cap, (1,), engages_at_the_cap),
    "at_the_cap-3": (at_the_cap, (3,), engages_at_the_cap),
    "one_past_the_cap-1": (at_the_cap, (1, True), engages_at_the_cap),
    "one_past_the_cap-3": (at_the_cap, (3, True), engages_at_the_cap),
    "round_robin-1": (round_robin, (1,), engages_round_robin),
    "round_robin-3": (round_robin, (3,), engages_round_robin),
    "many_words-1": (many_words, (1,), engages_many_words),
    "many_words-3": (many_words, (3,), engages_many_words),
}


def get(name):
    """(case, references of its evaluations), checked: the case reaches what it is named for, and every evaluation's count equals the older
    numpy count (tests/test_scan_rows_gpu.numpy_count) and is at least 1 wherever the pass is allowed."""
    make, args, engages = CASES[name]
    case = make(*args)
    refs = references(case)
    engages(case, refs)
    for (fA, fBs), ref in zip(case["evals"], refs):
        assert ref["count"] == numpy_count(case["P"], case["state"], fA, fBs) and ref["count"] >= 1
    return case, refs
