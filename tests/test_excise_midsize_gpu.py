"""graal_block_excisions at mid-size shapes against the windowed restatement (tests/excise_reference.Window): windows of more than two
64-fragment steps per walk, spans of 1 to 400 fragments with lengths around the wave width, spans at a head and at a tail, short flanks
on both sides, a span longer than two windows, a span whose excision brings contacts from beyond d_max inside the window, two
neighbouring spans with contacts between them and a contact around both, every fragment of three contigs a span of its own in one call,
a run of one span's contacts that crosses a wave, the whole 8,401-fragment contig and a ring.  check_branches() shows on the CPU that
the spans reach the branch they are named for: it is a test of its own without a GPU and runs again in front of every launch.

m2 (3,000 bins of three sub-fragments with RF counts 1..4, every 4th bin reversed) runs with the trans-branch indexing off and on, and
with it on some span must differ from its value with it off: the quirk term is reached.  m2 has no ring and no span that owns more than
64 consecutive contacts of the row-sorted list (see tests/test_flips_midsize_gpu.py).  Neither problem holds a contact further apart
than two windows: the spans longer than that have closing mass and no closing contact, and the contacts that come from beyond d_max are
shown on spans of 65 to 129 fragments (on m1's 129-fragment span 32 of the 33 contacts that feed its closing sum)."""
import numpy as np
import pytest

from graal_amd.lib import EXCISE_CIRCULAR, EXCISE_VALID, EXCISE_WHOLE
from tests import excise_reference as XR
from tests import link_reference as LR
from tests import window_cases
from tests.test_flips_midsize_gpu import crossing_row
from tests.test_scaffold_gpu import engine_for

# (call, contig by decreasing length, the span's first position, its last -- negative: counted from the contig's end --, tags)
M1_SPANS = ((0, 0, 0, 30, "head"), (0, 0, 600, 663, "interior"), (0, 0, 1000, 1064, "interior"), (0, 0, 1400, 1528, "interior closing"),
            (0, 0, 3000, 3399, "interior long"), (0, 0, 5000, 5099, "interior closing"), (0, 0, -301, -1, "tail"),
            (0, 1, 1, 64, "flank1"), (0, 4, 20, 40, "short_flanks"), (0, 2, 10, 20, "ring"),
            (2, 0, 0, -1, "whole"), (2, 5, 0, -1, "whole"), (2, 1, 7, 7, "one"))
M2_SPANS = ((0, 0, 0, 30, "head"), (0, 0, 300, 363, "interior"), (0, 0, 480, 544, "interior closing"), (0, 0, 700, 959, "long"), (0, 0, -60, -1, "tail"),
            (0, 1, 1, 64, "flank1"), (0, 1, 300, 428, "interior"), (0, 2, 250, 309, "interior"),
            (0, 3, 80, 419, "long short_flanks"), (1, 3, 0, -1, "whole"), (1, 2, 5, 5, "one"))
EVERY = {"m1": (3, 4, 5), "m2": ()}     # the contigs whose every fragment is a span of its own in one more call

_CACHE = {}


def bins_of(P):
    sid = np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)
    bin_of = np.zeros(int(sid[:, 3].sum()), np.int64)
    for w in range(3):
        bin_of[sid[sid[:, 3] > w, w]] = np.nonzero(sid[:, 3] > w)[0]
    return bin_of


def neighbours(P, s, m, lo, hi):
    """The position p in contig m, lo <= p < hi, of a one-fragment span p and a two-fragment span p + 3 .. p + 4 with a contact between
    them and a contact from a fragment before p to a fragment behind p + 4 at most 8 positions further on: it closes under both."""
    pos, idc = np.asarray(s["pos"]), np.asarray(s["id_c"])
    bin_of = bins_of(P)
    a, b = bin_of[np.asarray(P["coo_row"])], bin_of[np.asarray(P["coo_col"])]
    k = (idc[a] == idc[m[0]]) & (idc[b] == idc[m[0]])
    pa, pb = np.minimum(pos[a[k]], pos[b[k]]), np.maximum(pos[a[k]], pos[b[k]])
    for p in range(lo, hi):
        if ((pa == p) & (pb >= p + 3) & (pb <= p + 4)).any() and ((pa < p) & (pb > p + 4) & (pb - pa <= 12)).any():
            return p
    raise AssertionError("no such pair of neighbouring spans")


def problem(name):
    if name not in _CACHE:
        P = window_cases.m1(d_max=25.0) if name == "m1" else window_cases.m2()
        s = P["S_o_A_frags"]
        contigs = sorted(LR.contigs_of(s).values(), key=lambda m: -len(m))
        spec = list(M1_SPANS if name == "m1" else M2_SPANS)
        p = neighbours(P, s, contigs[0], 2000, 2400) if name == "m1" else neighbours(P, s, contigs[1], 100, 250)
        c = 0 if name == "m1" else 1
        spec += [(0, c, p, p, "near"), (0, c, p + 3, p + 4, "near")]
        if name == "m1":
            p0, p1 = crossing_row(P, contigs[3], 20, 180)
            spec.append((0, 3, p0, p1, "run64"))
        for c in EVERY[name]:
            spec += [(1, c, i, i, "every") for i in range(len(contigs[c]))]
        rows = []
        for call, c, p0, p1, tags in spec:
            m = contigs[c]
            p0, p1 = (p if p >= 0 else len(m) + p for p in (p0, p1))
            rows.append((int(m[p0]), int(m[p1]), c, p0, p1, tags, call))
        _CACHE[name] = (P, s, contigs, rows, {})
    return _CACHE[name]


def calls_of(rows):
    """Per call: (indices into rows, first, last)."""
    out = []
    for call in sorted({r[6] for r in rows}):
        k = [i for i, r in enumerate(rows) if r[6] == call]
        out.append((k,) + tuple(np.array([rows[i][j] for i in k], np.int32) for j in range(2)))
    return out


def reference(name, quirk):
    """(q, contacts, status, A) and the restatement's parts per call, once per (problem, mode)."""
    P, s, contigs, rows, refs = problem(name)
    if quirk not in refs:
        W = XR.window(P, quirk=quirk)
        refs[quirk] = []
        for _, first, last in calls_of(rows):
            parts = {}
            refs[quirk].append(W.excisions(s, first, last, parts) + (parts,))
    return refs[quirk]


def check_branches(name):
    """The spans reach the branches their tags name (CPU)."""
    P, s, contigs, rows, _ = problem(name)
    start, ln = np.asarray(s["start_bp"], np.int64), np.asarray(s["len_bp"], np.int64)
    reach = XR.window(P).reach
    row, col = np.asarray(P["coo_row"]), np.asarray(P["coo_col"])
    bin_of = bins_of(P)
    refs = reference(name, False)
    calls = calls_of(rows)
    parts0 = refs[0][4]
    at = {j: i for i, j in enumerate(calls[0][0])}                          # row index -> index in call 0
    sp = np.full(len(start), -1)
    near, lens = [], []
    for k, (f, l, c, p0, p1, tags, call) in enumerate(rows):
        m = contigs[c]
        assert 0 <= p0 <= p1 < len(m)
        s0, e1 = start[f], start[l] + ln[l]
        left, right = s0 - start[m[0]], start[m[-1]] + ln[m[-1]] - e1
        if call != 1:
            lens.append(p1 - p0 + 1)
        if "interior" in tags:
            assert left > reach and right > reach
            n_win = int(np.searchsorted(start[m], s0 + reach) - p0)
            assert n_win > (128 if name == "m1" else 90)                      # (m1: more than two 64-fragment steps in every walk)
        if "long" in tags:
            assert e1 - s0 > 2 * reach + 4000                                    # fragments of X out of reach of both its ends
            # (every L x R pair is beyond the window now: its mass moves from v_inter to the price of new neighbours, and every contact
            # that feeds the closing sum comes from beyond d_max)
            assert parts0["closing_mass"][at[k]] != 0 and parts0["closing_fed"][at[k]] == parts0["closing_from_outside"][at[k]]
        if "closing" in tags:
            assert parts0["closing_from_outside"][at[k]] > 0                     # a contact at >= d_max now, below it afterwards
        if "head" in tags:
            assert p0 == 0 and p1 < len(m) - 1
        if "tail" in tags:
            assert p1 == len(m) - 1 and p0 > 0
        if "flank1" in tags:
            assert p0 == 1
        if "short_flanks" in tags:
            assert 0 < left < reach and 0 < right < reach
        if "whole" in tags:
            assert p0 == 0 and p1 == len(m) - 1
        if "one" in tags:
            assert p0 == p1
        assert ("ring" in tags) == (np.asarray(s["circ"])[f] == 1)
        if "near" in tags:
            near.append(k)
        if "ring" not in tags and call == 0:
            assert (sp[m[p0:p1 + 1]] == -1).all()
            sp[m[p0:p1 + 1]] = k
    a, b = near
    assert 0 < start[rows[b][0]] - (start[rows[a][1]] + ln[rows[a][1]]) < reach
    ka, kb = sp[bin_of[row]], sp[bin_of[col]]
    assert (((ka == a) & (kb == b)) | ((ka == b) & (kb == a))).sum() > 0   # contacts between the two neighbouring spans
    assert parts0["closing_fed"][at[a]] > 0 and parts0["closing_fed"][at[b]] > 0
    pos, idc = np.asarray(s["pos"]), np.asarray(s["id_c"])
    ra, rb = bin_of[row], bin_of[col]
    same = idc[ra] == idc[rows[a][0]]
    lo_, hi_ = np.minimum(pos[ra], pos[rb]), np.maximum(pos[ra], pos[rb])
    assert (same & (idc[rb] == idc[ra]) & (lo_ < rows[a][3]) & (hi_ > rows[b][4]) & (hi_ - lo_ <= 12)).any()   # one contact, two closing sums
    assert {1, 2, 64, 65, 129} <= set(lens)
    if name == "m1":
        assert any("whole" in r[5] and len(contigs[r[2]]) == 8401 for r in rows) and any("ring" in r[5] for r in rows)
        assert sorted(len(contigs[c]) for c in EVERY[name]) == [36, 63, 200]
        fed = refs[1][4]["closing_fed"]
        assert len(fed) == 299 and np.median(fed) > 20                          # a near-diagonal contact feeds many spans' sums
        k = [i for i, r in enumerate(rows) if "run64" in r[5]][0]
        same = idc[ra] == idc[rb]
        key = np.where(same & (ka != kb), ka, -1)                            # the row side's span, as the contact pass keys its runs
        idx = np.nonzero(key == k)[0]
        assert len(idx) > 64 and (np.diff(idx) == 1).all() and idx[0] // 64 != idx[-1] // 64
    return reach


@pytest.mark.parametrize("name", ["m1", "m2"])
def test_cases_reach_their_branches(name):
    assert check_branches(name) > 0


def test_the_mode_reaches_the_quirk_term_on_m2():
    """With the indexing on, spans of m2 differ from their value with it off, in the contacts, in the mass inside the window and in the
    far pairs (the quirk term proper)."""
    off, on = reference("m2", False)[0], reference("m2", True)[0]
    assert (off[0] != on[0]).any()
    assert (on[4]["far"] != 0).any() and not (off[4]["far"] != 0).any()


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
        for _, first, last in calls:
            perm = rng.permutation(len(first))
            got.append((e.block_excisions_q(first, last), perm, e.block_excisions_q(first[perm], last[perm])))
    finally:
        e.close()
    n_evidence = 0
    for (k, first, last), (rq, rc, rst, A, _), ((q, c, st), perm, (q2, c2, st2)) in zip(calls, refs, got):
        for i, j in enumerate(k):
            tags = rows[j][5]
            assert rst[i] == (EXCISE_CIRCULAR if "ring" in tags else EXCISE_WHOLE if "whole" in tags else EXCISE_VALID), rows[j]
        print(name, quirk, len(first), "spans: max |q - rq|", int(np.max(np.abs(q - rq))), "max A", int(A.max()))
        assert np.array_equal(st, rst) and np.array_equal(c, rc), (st, rst, c, rc)
        assert np.all(np.abs(q - rq) <= 1e-9 * A + 1), (np.abs(q - rq), A)
        assert (rq[rst == EXCISE_VALID] != 0).all()
        n_evidence += int((rc[rst == EXCISE_VALID] > 0).sum())
        assert np.array_equal(q[perm], q2) and np.array_equal(c[perm], c2) and np.array_equal(st[perm], st2)
    assert n_evidence >= 8
    if quirk:                                                                # (at least one span differs from its value with the mode off)
        assert any((rq != rq0).any() for (rq, *_), (rq0, *_) in zip(refs, reference(name, False)))
