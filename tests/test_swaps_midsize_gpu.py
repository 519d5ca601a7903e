"""graal_block_swaps at mid-size shapes against the windowed restatement (tests/swap_reference.Window): windows of more than two
64-fragment steps per walk, runs of 1 to 2,000 fragments with lengths around the wave width, runs longer than two windows, a span that is
its whole 8,401-fragment contig, X at a contig's head and Y at a tail, short flanks, neighbouring swaps with contacts between them, and a
run of one swap's contacts that crosses a wave.  check_branches() shows on the CPU that the swaps reach the branch they are named for:
it is a test of its own without a GPU and runs again in front of every launch.

m2 (3,000 bins of three sub-fragments) runs with the trans-branch indexing off and on; it has no ring and no swap that owns more than
64 consecutive contacts of the row-sorted list (see tests/test_flips_midsize_gpu.py)."""
import numpy as np
import pytest

from graal_amd.lib import SWAP_CIRCULAR, SWAP_VALID
from tests import link_reference as LR
from tests import swap_reference as SR
from tests import window_cases
from tests.test_flips_midsize_gpu import crossing_row
from tests.test_scaffold_gpu import engine_for

# (call, contig by decreasing length, X's first position, X's last, Y's last -- negative: counted from the contig's end --, tags)
M1_SWAPS = ((0, 0, 0, 30, 62, "head"), (0, 0, 100, 100, 101, "near one"), (0, 0, 104, 105, 107, "near"), (0, 0, 600, 663, 727, "interior"),
            (0, 0, 1000, 1064, 1128, "interior"), (0, 0, 1400, 1527, 1656, "interior"), (0, 0, 2000, 2199, 2500, "interior window"),
            (0, 0, 3000, 4999, 5400, "interior long"), (0, 0, -301, -101, -1, "tail"),
            (0, 1, 1, 64, 130, "flank1"), (0, 1, -50, -36, -21, "short_flank"), (0, 4, 0, 30, -1, "whole"), (0, 5, 0, 0, -1, "whole"),
            (0, 2, 10, 20, 40, "ring"),
            (1, 0, 0, 4000, -1, "whole long"), (1, 1, 7, 7, 8, "one"))
M2_SWAPS = ((0, 0, 0, 30, 62, "head"), (0, 0, 100, 100, 101, "near one"), (0, 0, 104, 105, 107, "near"), (0, 0, 300, 363, 427, "interior"),
            (0, 0, 480, 544, 609, "interior"), (0, 0, 700, 959, 1030, "long"), (0, 0, -60, -30, -1, "tail"),
            (0, 1, 1, 64, 129, "flank1"), (0, 1, 300, 428, 557, "interior"), (0, 1, -40, -30, -21, "short_flank"),
            (0, 2, 50, 349, 549, "long short_flank"), (0, 3, 0, 249, -1, "whole"))

_CACHE = {}


def problem(name):
    if name not in _CACHE:
        P = window_cases.m1(d_max=25.0) if name == "m1" else window_cases.m2()
        s = P["S_o_A_frags"]
        contigs = sorted(LR.contigs_of(s).values(), key=lambda m: -len(m))
        spec = list(M1_SWAPS if name == "m1" else M2_SWAPS)
        if name == "m1":
            p0, p1 = crossing_row(P, contigs[3], 20, 180)
            spec.append((0, 3, p0, p0, p1, "run64 one"))
        rows = []
        for call, c, p0, pm, p1, tags in spec:
            m = contigs[c]
            p0, pm, p1 = (p if p >= 0 else len(m) + p for p in (p0, pm, p1))
            rows.append((int(m[p0]), int(m[pm]), int(m[p1]), c, p0, pm, p1, tags, call))
        _CACHE[name] = (P, s, contigs, rows, {})
    return _CACHE[name]


def calls_of(rows):
    """Per call: (indices into rows, first, mid, last)."""
    out = []
    for call in sorted({r[8] for r in rows}):
        k = [i for i, r in enumerate(rows) if r[8] == call]
        out.append((k,) + tuple(np.array([rows[i][j] for i in k], np.int32) for j in range(3)))
    return out


def reference(name, quirk):
    P, s, contigs, rows, refs = problem(name)
    if quirk not in refs:
        W = SR.window(P, quirk=quirk)
        refs[quirk] = [W.swaps(s, first, mid, last) for _, first, mid, last in calls_of(rows)]
    return refs[quirk]


def check_branches(name):
    """The swaps reach the branches their tags name (CPU)."""
    P, s, contigs, rows, _ = problem(name)
    start, ln = np.asarray(s["start_bp"], np.int64), np.asarray(s["len_bp"], np.int64)
    reach = SR.window(P).reach
    row, col = np.asarray(P["coo_row"]), np.asarray(P["coo_col"])
    sid = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
    bin_of = np.zeros(int(sid[:, 3].sum()), np.int64)
    for w in range(3):
        bin_of[sid[sid[:, 3] > w, w]] = np.nonzero(sid[:, 3] > w)[0]
    sw = np.full(len(start), -1); role = np.zeros(len(start), np.int64)
    near, lens = [], []
    for k, (f, mi, l, c, p0, pm, p1, tags, call) in enumerate(rows):
        m = contigs[c]
        assert 0 <= p0 <= pm < p1 < len(m)
        s0, sm, e1 = start[f], start[mi] + ln[mi], start[l] + ln[l]
        left, right = s0 - start[m[0]], start[m[-1]] + ln[m[-1]] - e1
        lens += [pm - p0 + 1, p1 - pm]
        if "window" in tags:
            n_win = int(np.searchsorted(start[m], s0 + reach) - p0)
            assert n_win > 128 and pm - p0 + 1 > n_win and p1 - pm > n_win        # more than two 64-fragment steps in every walk
        if "interior" in tags:
            assert left > reach and right > reach
        if "long" in tags:
            assert sm - s0 > 2 * reach + 4000                                    # fragments of X out of reach of both its ends
        if "head" in tags:
            assert p0 == 0 and p1 < len(m) - 1
        if "tail" in tags:
            assert p1 == len(m) - 1 and p0 > 0
        if "flank1" in tags:
            assert p0 == 1
        if "short_flank" in tags:
            assert 0 < min(left, right) < reach and p0 > 1 and p1 < len(m) - 2
        if "whole" in tags:
            assert p0 == 0 and p1 == len(m) - 1
        if "one" in tags:
            assert p0 == pm and p1 == pm + 1
        assert ("ring" in tags) == (np.asarray(s["circ"])[f] == 1)
        if "near" in tags:
            near.append(k)
        if "ring" not in tags and call == 0:
            assert (sw[m[p0:p1 + 1]] == -1).all()
            sw[m[p0:p1 + 1]] = k; role[m[pm + 1:p1 + 1]] = 1
    a, b = near
    assert 0 < start[rows[b][0]] - (start[rows[a][2]] + ln[rows[a][2]]) < reach
    ka, kb = sw[bin_of[row]], sw[bin_of[col]]
    assert ((ka == a) & (kb == b)).sum() > 0                               # contacts between the two neighbouring swaps
    assert {1, 2, 64, 65, 129} <= set(lens)
    if name == "m1":
        assert {128, 200, 2000} <= set(lens) and any("whole" in r[7] and len(contigs[r[3]]) == 8401 for r in rows)
        k = [i for i, r in enumerate(rows) if "run64" in r[7]][0]
        same = np.asarray(s["id_c"])[bin_of[row]] == np.asarray(s["id_c"])[bin_of[col]]
        ra, rb = role[bin_of[row]], role[bin_of[col]]
        key = np.where(same & ((ka != kb) | ((ka >= 0) & (ra != rb))), ka, -1)   # the row side's swap, as the contact pass keys its runs
        idx = np.nonzero(key == k)[0]
        assert len(idx) > 64 and (np.diff(idx) == 1).all() and idx[0] // 64 != idx[-1] // 64
    return reach


@pytest.mark.parametrize("name", ["m1", "m2"])
def test_cases_reach_their_branches(name):
    assert check_branches(name) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,quirk", [("m1", False), ("m2", False), ("m2", True)])
def test_equals_windowed_reference(name, quirk):
    check_branches(name)
    P, s, contigs, rows, _ = problem(name)
    refs = reference(name, quirk)
    calls = calls_of(rows)
    rng = np.random.RandomState(11)
    got = []
    e = engine_for(P, quirk=quirk)
    try:
        for _, first, mid, last in calls:
            perm = rng.permutation(len(first))
            got.append((e.block_swaps_q(first, mid, last), perm, e.block_swaps_q(first[perm], mid[perm], last[perm])))
    finally:
        e.close()
    n_evidence = 0
    for (k, first, mid, last), (rq, rc, rst, A), ((q, c, st), perm, (q2, c2, st2)) in zip(calls, refs, got):
        for i, j in enumerate(k):
            assert rst[i] == (SWAP_CIRCULAR if "ring" in rows[j][7] else SWAP_VALID), rows[j]
        assert np.array_equal(st, rst) and np.array_equal(c, rc), (st, rst, c, rc)
        assert np.all(np.abs(q - rq) <= 1e-9 * A + 1), (np.abs(q - rq), A)
        assert (rq[rst == SWAP_VALID] != 0).all()
        n_evidence += int((rc[rst == SWAP_VALID] > 0).sum())
        assert np.array_equal(q[perm], q2) and np.array_equal(c[perm], c2) and np.array_equal(st[perm], st2)
    assert n_evidence >= 8
    if quirk:                                                                # (the mode changes nothing: the same integers as with it off)
        for (rq, rc, rst, A), (rq0, rc0, rst0, A0) in zip(refs, reference(name, False)):
            assert np.array_equal(rq, rq0) and np.array_equal(rc, rc0)
