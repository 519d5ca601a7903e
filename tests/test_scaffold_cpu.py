"""CPU: the numpy restatement of graal_edit_layout (tests/edit_reference.py) against link_reference.join_layout and
junction_reference.cut_layout, the cycle breaker and the round logic of graal_amd.scaffold on hand-built tables, and the TSV writer."""
import os
import tempfile

import numpy as np
import pytest

from graal_amd import scaffold
from graal_amd.lib import EDIT_CIRCULAR, EDIT_CYCLE, EDIT_END_TWICE, EDIT_SAME_CONTIG, Q_SCALE
from tests import edit_reference as ER
from tests import link_reference as LR
from tests.junction_reference import cut_layout

FIELDS = LR.FIELDS


def random_layout(rng, n=40, n_contigs=6, ring=False):
    lens = rng.randint(500, 3000, size=n)
    perm = rng.permutation(n)
    cuts = np.sort(rng.choice(np.arange(5 if ring else 1, n), n_contigs - 1, replace=False))   # (a ring of >= 5 fragments)
    contigs = [[(int(f), int(rng.choice([-1, 1]))) for f in part] for part in np.split(perm, cuts)]
    return LR.layout(lens, contigs, {0} if ring else ())


def same(a, b, keys=FIELDS):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def ends(state):
    return {c: (2 * int(m[0]), 2 * int(m[-1]) + 1) for c, m in LR.contigs_of(state).items()}


@pytest.mark.parametrize("seed", range(6))
def test_single_join_equals_join_layout(seed):
    rng = np.random.RandomState(seed)
    s = random_layout(rng)
    E = ends(s)
    ca, cb = rng.choice(sorted(E), 2, replace=False)
    ea, eb = sorted((E[ca][rng.randint(2)], E[cb][rng.randint(2)]))
    got, st = ER.edit(s, [], [(eb, ea)])
    assert st is not None and not st.any()
    want = LR.join_layout(s, ea, eb)
    lab_a, lab_b = int(s["id_c"][ea >> 1]), int(s["id_c"][eb >> 1])
    joined = want["id_c"] == lab_a
    want["id_c"][joined] = min(lab_a, lab_b)          # (the documented label: the lowest of the two)
    same(got, want)


def end_now(state, f):
    """The end of fragment f in `state` (f must be an end fragment of a contig of >= 2 fragments)."""
    return 2 * f + (1 if int(state["pos"][f]) == int(state["l_cont"][f]) - 1 else 0)


@pytest.mark.parametrize("seed", range(8))
def test_chain_equals_successive_joins(seed):
    """3 to 5 contigs joined in one edit equal join_layout applied join by join along the chain, with the chain in its canonical direction
    (the contig of the lowest joined end before its partner) and the lowest label."""
    rng = np.random.RandomState(100 + seed)
    s = random_layout(rng, n=60, n_contigs=8)
    multi = [c for c, m in LR.contigs_of(s).items() if len(m) >= 2]
    labs = [int(c) for c in rng.permutation(multi)[:3 + seed % 3]]
    E = ends(s)
    joins, chain_ends, prev_exit = [], [], None
    for c in labs:
        h, t = E[c]
        entry, exit_ = (h, t) if rng.rand() < 0.5 else (t, h)
        if prev_exit is not None:
            joins.append((prev_exit, entry) if rng.rand() < 0.5 else (entry, prev_exit))
        chain_ends.append((entry, exit_))
        prev_exit = exit_
    order = [joins[k] for k in rng.permutation(len(joins))]
    got, st = ER.edit(s, [], order)
    assert not st.any()
    # fold join_layout along the chain: the growing contig's exit end, then the next contig's entry end, in the CURRENT layout
    cur = {k: np.array(v) for k, v in s.items()}
    for i in range(1, len(labs)):
        x = end_now(cur, chain_ends[i - 1][1] >> 1)
        y = end_now(cur, chain_ends[i][0] >> 1)
        cur = LR.join_layout(cur, min(x, y), max(x, y))
    frags = [f for c in labs for f in LR.contigs_of(s)[c]]
    chain = LR.contig_lists(cur)[int(cur["id_c"][frags[0]])]
    e_min = min(e for j in joins for e in j)
    partner = dict([(a, b) for a, b in joins] + [(b, a) for a, b in joins])[e_min]
    idx = {f: k for k, (f, _) in enumerate(chain)}
    if idx[e_min >> 1] > idx[partner >> 1]:
        chain = [(f, -o) for f, o in reversed(chain)]
    want = LR.layout(s["len_bp"], [chain])
    got_chain = LR.contig_lists(got)[int(got["id_c"][frags[0]])]
    assert got_chain == chain
    m = [f for f, _ in chain]
    for k in ("pos", "start_bp", "ori", "prev", "next", "l_cont", "l_cont_bp", "circ"):
        assert np.array_equal(got[k][m], np.asarray(want[k])[m]), k
    assert set(got["id_c"][m].tolist()) == {min(labs)}
    rest = np.setdiff1d(np.arange(len(s["id_c"])), m)
    for k in FIELDS:
        assert np.array_equal(got[k][rest], np.asarray(s[k])[rest]), k


@pytest.mark.parametrize("seed", range(6))
def test_cuts_equal_cut_layout(seed):
    rng = np.random.RandomState(200 + seed)
    s = random_layout(rng)
    inner = [f for f in range(len(s["id_c"])) if s["pos"][f] < s["l_cont"][f] - 1]
    f = int(rng.choice(inner))
    got, st = ER.edit(s, [f], [])
    assert not st.any()
    same(got, cut_layout(s, f))
    # two cuts one after the other: the second piece's label is the next fresh one in order of first fragment
    g = [x for x in inner if x != f and s["id_c"][x] != s["id_c"][f]]
    if g:
        f2 = int(g[0])
        got2, _ = ER.edit(s, [f, f2], [])
        heads = sorted([int(s["next"][f]), int(s["next"][f2])])
        mx = int(s["id_c"].max())
        assert [int(got2["id_c"][h]) for h in heads] == [mx + 1, mx + 2]


def test_ring_cut_opens_at_the_next_fragment():
    rng = np.random.RandomState(3)
    s = random_layout(rng, ring=True)
    ring = LR.contigs_of(s)[0]
    f = int(ring[2])
    got, st = ER.edit(s, [f], [])
    assert not st.any()
    m = LR.contigs_of(got)[0]
    assert int(m[0]) == int(ring[3]) and int(m[-1]) == f and got["circ"][m].max() == 0
    assert list(got["start_bp"][m]) == list(np.concatenate([[0], np.cumsum(s["len_bp"][m])[:-1]]))


def test_refusals():
    rng = np.random.RandomState(4)
    s = random_layout(rng, ring=True)
    E = ends(s)
    a, b = E[1], E[2]
    assert ER.edit(s, [], [(a[0], a[1])])[1][0] == EDIT_SAME_CONTIG
    assert ER.edit(s, [], [(a[1], b[0]), (a[1], E[3][0])])[1].tolist() == [EDIT_END_TWICE, EDIT_END_TWICE]
    assert ER.edit(s, [], [(2 * int(LR.contigs_of(s)[0][0]), b[0])])[1][0] == EDIT_CIRCULAR
    st = ER.edit(s, [], [(a[1], b[0]), (b[1], E[3][0]), (E[3][1], a[0])])[1]
    assert st.tolist() == [EDIT_CYCLE] * 3


def test_break_cycles_drops_the_weakest_join():
    contig = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 2, 6: 3, 7: 3}.__getitem__
    ea, eb = [1, 3, 5], [2, 4, 0]             # contigs 0-1, 1-2, 2-0: a cycle
    keep = scaffold.break_cycles(ea[:3], eb[:3], [3.0, 1.0, 2.0], contig)
    assert keep.tolist() == [True, False, True]
    keep = scaffold.break_cycles(ea[:2], eb[:2], [3.0, 1.0], contig)
    assert keep.tolist() == [True, True]
    # ties: the larger (end_a, end_b) is the weaker -- (3, 4) against (0, 5) and (1, 2)
    keep = scaffold.break_cycles(ea[:3], eb[:3], [1.0, 1.0, 1.0], contig)
    assert keep.tolist() == [True, False, True]


def test_plan_joins_filters_scores_and_breaks_cycles():
    contig = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 5: 2}.__getitem__
    q = (np.array([3.0, 1.0, 2.0, -1.0]) * Q_SCALE).astype(np.int64)
    a, b, sc = scaffold.plan_joins((np.array([1, 3, 0, 2]), np.array([2, 4, 5, 5]), q), 0.0, contig)
    assert list(zip(a.tolist(), b.tolist())) == [(1, 2), (0, 5)]
    a, b, _ = scaffold.plan_joins((np.array([1, 3, 0]), np.array([2, 4, 5]), q[:3]), 2.5, contig)
    assert list(zip(a.tolist(), b.tolist())) == [(1, 2)]


class FakeEngine(scaffold.Engine):
    """The engine calls of scaffold() on a layout in numpy: end_links_best from a fixed table of mutual links per round, edit_layout
    through the restatement, eval_full from a fixed series."""

    def __init__(self, state, mutual_rounds, logls):
        self.s, self.mutual, self.logls, self.calls = state, list(mutual_rounds), list(logls), []

    def relabel_contigs(self):
        return int(self.s["id_c"].max())

    def eval_full(self):
        return self.logls.pop(0)

    def download_frags(self):
        return {k: np.array(v) for k, v in self.s.items()}

    def upload_frags(self, s):
        self.calls.append("upload")
        self.s = {k: np.array(v) for k, v in s.items()}

    def end_links_best(self, min_frags=1):
        a, b, q = self.mutual.pop(0) if self.mutual else ([], [], [])
        return None, None, (np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32), (np.asarray(q, dtype=np.float64) * Q_SCALE).astype(np.int64))

    def edit_layout(self, cuts=(), joins=()):
        self.calls.append(("edit", len(cuts), len(joins)))
        new, st = ER.edit(self.s, cuts, joins)
        assert new is not None, st
        self.s = new
        return st

    def junction_scores(self):
        raise AssertionError("not asked for")


def test_rounds_stop_when_no_join_remains_and_undo_a_worse_round():
    rng = np.random.RandomState(5)
    s = random_layout(rng, n=30, n_contigs=5)
    E = ends(s)
    r1 = ([E[0][1]], [E[1][0]], [2.0])
    e = FakeEngine(s, [r1], [-100.0, -90.0])
    rec = scaffold.scaffold(e, rounds=10)
    assert [r["round"] for r in rec] == [0, 1] and rec[1]["joins"] == 1 and rec[1]["contigs"] == 4
    assert e.calls == [("edit", 0, 1)]
    # a round that lowers logL is undone and ends the run
    e = FakeEngine(s, [r1, ([E[2][1]], [E[3][0]], [1.0])], [-100.0, -90.0, -95.0, -90.0])
    rec = scaffold.scaffold(e, rounds=10)
    assert [(r["round"], r["kept"]) for r in rec] == [(0, 1), (1, 1), (2, 0)]
    assert e.calls[-1] == "upload" and len(LR.contigs_of(e.s)) == 4


def test_write_scaffold_tsv():
    rec = [{"round": 0, "cuts": 0, "joins": 0, "contigs": 9, "logL": -12.5, "kept": 1},
           {"round": 1, "cuts": 2, "joins": 5, "contigs": 6, "logL": -3.0000000000000004, "kept": 1}]
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.tsv")
        assert scaffold.write_scaffold_tsv(p, rec) == 2
        lines = open(p).read().splitlines()
    assert lines[0].split("\t") == list(scaffold.COLUMNS)
    assert lines[2].split("\t") == ["1", "2", "5", "6", "-3.0000000000000004", "1"]
