"""graal_block_flips at mid-size shapes against the windowed restatement (tests/flip_reference.Window): windows of more than two
64-fragment steps, blocks of every length around the wave width, blocks longer than two windows, blocks at a contig's head and tail and
with short flanks, neighbouring blocks with contacts between them, and a run of one block's contacts that crosses a wave.  Every case
first checks on the CPU that its blocks reach the branch they are named for.

m2 runs m1's list scaled to its window, less two cases it cannot give: it has no ring, and no block of it owns more than 64 consecutive
contacts of the row-sorted list (its rows are sub-fragments of at most 27 contacts, and a block's rows are interrupted by the contacts
inside the block and with other contigs: the longest run any block of 1 to 8 bins owns is 31)."""
import numpy as np
import pytest

from graal_amd.lib import FLIP_CIRCULAR, FLIP_VALID, FLIP_WHOLE
from tests import flip_reference as FR
from tests import link_reference as LR
from tests import window_cases
from tests.test_scaffold_gpu import engine_for

pytestmark = pytest.mark.gpu

# (contig by decreasing length, first position, last position or negative: counted from the contig's end, tags)
M1_BLOCKS = ((0, 0, 62, "head"), (0, 100, 100, "near"), (0, 120, 121, "near"), (0, 600, 663, "interior"), (0, 1000, 1064, "interior"),
             (0, 1400, 1527, "interior"), (0, 1900, 2028, "interior"), (0, 2400, 2569, "interior window"), (0, 3000, 3399, "interior long"),
             (0, 4000, 5999, "interior long"), (0, -101, -1, "tail"),
             (1, 1, 130, "flank1"), (1, -50, -21, "short_flank"), (4, 0, 61, "head"), (4, 62, 62, "tail"), (5, 0, -1, "whole"),
             (2, 10, 40, "ring"))
M2_BLOCKS = ((0, 0, 62, "head"), (0, 100, 100, "near"), (0, 104, 105, "near"), (0, 300, 363, "interior"), (0, 480, 544, "interior"),
             (0, 700, 959, "interior long"), (0, -60, -1, "tail"),
             (1, 1, 128, "flank1"), (1, 300, 428, "interior"), (1, 580, 689, "window"), (1, -40, -21, "short_flank"),
             (2, 50, 549, "long short_flank"), (3, 0, -1, "whole"))

_CACHE = {}


def problem(name):
    if name not in _CACHE:
        P = window_cases.m1(d_max=25.0) if name == "m1" else window_cases.m2()
        s = P["S_o_A_frags"]
        contigs = sorted(LR.contigs_of(s).values(), key=lambda m: -len(m))
        spec = list(M1_BLOCKS if name == "m1" else M2_BLOCKS)
        if name == "m1":
            spec.append((3, *crossing_row(P, contigs[3], 20, 180), "run64"))
        blocks = []
        for c, p0, p1, tags in spec:
            m = contigs[c]
            p0, p1 = (p0 if p0 >= 0 else len(m) + p0), (p1 if p1 >= 0 else len(m) + p1)
            blocks.append((int(m[p0]), int(m[p1]), c, p0, p1, tags))
        _CACHE[name] = (P, s, contigs, blocks, {})
    return _CACHE[name]


def crossing_row(P, m, lo, hi):
    """A two-fragment block (its positions) of contig m between positions lo and hi whose two rows of the (row, col)-sorted list are
    consecutive contacts of its contig, more than a wave of them: the first row holds no contact with another contig."""
    row, col = np.asarray(P["coo_row"]), np.asarray(P["coo_col"])
    assert (np.diff(row) >= 0).all() and (np.diff(m) == 1).all()
    inside = (col >= m[0]) & (col <= m[-1])
    per_row = np.bincount(row[inside], minlength=int(m[-1]) + 2)
    total = np.bincount(row, minlength=int(m[-1]) + 2)
    f = m[lo:hi]
    ok = np.nonzero((total[f] == per_row[f]) & (per_row[f] + per_row[f + 1] > 70))[0]
    assert len(ok) > 0
    return lo + int(ok[0]), lo + int(ok[0]) + 1


def reference(name, quirk):
    P, s, contigs, blocks, refs = problem(name)
    if quirk not in refs:
        first, last = np.array([b[0] for b in blocks]), np.array([b[1] for b in blocks])
        refs[quirk] = FR.window(P, quirk=quirk).flips(s, first, last)
    return refs[quirk]


def check_branches(name):
    """The blocks reach the branches their tags name (CPU)."""
    P, s, contigs, blocks, _ = problem(name)
    start, ln = np.asarray(s["start_bp"], np.int64), np.asarray(s["len_bp"], np.int64)
    reach = WINDOW = FR.window(P).reach
    row, col = np.asarray(P["coo_row"]), np.asarray(P["coo_col"])
    sid = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
    bin_of = np.zeros(int(sid[:, 3].sum()), np.int64)
    for w in range(3):
        bin_of[sid[sid[:, 3] > w, w]] = np.nonzero(sid[:, 3] > w)[0]
    blk = np.full(len(start), -1)
    near = []
    for k, (f, l, c, p0, p1, tags) in enumerate(blocks):
        m = contigs[c]
        s0, e1 = start[f], start[l] + ln[l]
        left, right = s0 - start[m[0]], start[m[-1]] + ln[m[-1]] - e1
        n_win = int(np.searchsorted(start[m], s0 + reach) - p0)
        if "window" in tags and name == "m1":
            assert n_win > 128 and abs((p1 - p0 + 1) - n_win) < 20          # more than two 64-fragment steps per flank
        if "interior" in tags:
            assert left > reach and right > reach
        if "long" in tags:
            assert e1 - s0 > 2 * reach + 4000                              # fragments out of reach of both boundaries
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
        if "ring" in tags:
            assert np.asarray(s["circ"])[f] == 1
        if "near" in tags:
            near.append(k)
        if "whole" not in tags and "ring" not in tags:
            assert (blk[m[p0:p1 + 1]] == -1).all()
            blk[m[p0:p1 + 1]] = k
    a, b = near
    assert 0 < start[blocks[b][0]] - (start[blocks[a][1]] + ln[blocks[a][1]]) < reach
    ka, kb = blk[bin_of[row]], blk[bin_of[col]]
    assert ((ka == a) & (kb == b)).sum() > 0                               # contacts between the two neighbouring blocks
    lens = sorted(b[4] - b[3] + 1 for b in blocks)
    assert {1, 2, 63, 64, 65, 128, 129} <= set(lens)
    if name == "m1":
        assert {400, 2000, 62} <= set(lens)
        k = [i for i, b in enumerate(blocks) if "run64" in b[5]][0]
        same = np.asarray(s["id_c"])[bin_of[row]] == np.asarray(s["id_c"])[bin_of[col]]
        key = np.where(same & (ka != kb), ka, -1)                          # the row side's block, as the contact pass keys its runs
        idx = np.nonzero(key == k)[0]
        assert len(idx) > 64 and (np.diff(idx) == 1).all() and idx[0] // 64 != idx[-1] // 64
    return WINDOW


@pytest.mark.parametrize("name,quirk", [("m1", False), ("m2", False), ("m2", True)])
def test_equals_windowed_reference(name, quirk):
    check_branches(name)
    P, s, contigs, blocks, _ = problem(name)
    rq, rc, rst, A = reference(name, quirk)
    first, last = np.array([b[0] for b in blocks], np.int32), np.array([b[1] for b in blocks], np.int32)
    perm = np.random.RandomState(11).permutation(len(first))
    e = engine_for(P, quirk=quirk)
    try:
        q, c, st = e.block_flips_q(first, last)
        q2, c2, st2 = e.block_flips_q(first[perm], last[perm])
    finally:
        e.close()
    for k, b in enumerate(blocks):
        want = FLIP_WHOLE if "whole" in b[5] else FLIP_CIRCULAR if "ring" in b[5] else FLIP_VALID
        assert rst[k] == want, b
    assert np.array_equal(st, rst) and np.array_equal(c, rc), (st, rst, c, rc)
    assert np.all(np.abs(q - rq) <= 1e-9 * A + 1), (np.abs(q - rq), A)
    v = (rst == FLIP_VALID) & (first != last)                             # (a one-fragment block of a one-sub-fragment bin scores 0)
    assert (rq[v] != 0).all() and (rc[rst == FLIP_VALID] > 0).sum() >= 8
    if quirk:
        parts = {}
        FR.window(P, quirk=True).flips(s, first[:4], last[:4], parts)
        assert parts["mirror"].any() and parts["mirror_contacts"].any()   # (the mode's terms are in play)
    assert np.array_equal(q[perm], q2) and np.array_equal(c[perm], c2) and np.array_equal(st[perm], st2)
