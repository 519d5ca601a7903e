"""Transpositions: score swaps of two adjacent runs of a contig (Engine.block_swaps) and swap those the data prefer.

    tilings(soa, marks=None, max_units=8)                         -- disjoint swap sets (first, mid, last) that cover every short pair once
    plan_swaps(candidates, soa, reach_bp, min_score=0.0)          -- the swaps of a round: best first, no two within reach of each other
    swap_edit(soa, first, mid, last)                              -- the cuts and joins that apply those swaps (graal_edit_layout)
    swap_rounds(sampler_or_engine, max_frags=8, ...)              -- the rounds; returns their record
    score_table(engine, soa, sets) / write_swaps_tsv, write_swap_rounds_tsv

A swap names two adjacent runs X, Y of one linear contig; the swapped layout has Y in front of X inside the same bp interval, nothing
turned round.  Any move of a run inside its contig is a swap of that run with the adjacent run it passes, so this one score covers
every transposition.  graal_block_swaps scores every swap of a call alone, so the spans of a call must be disjoint: "every pair of
adjacent runs of at most N units together" is the sum over m = 2 .. N of m (m - 1) tilings (span m, split a = 1 .. m - 1, offset
0 .. m - 1).  A UNIT is a fragment (marks=None) or a maximal run between marked junctions (flips.weak_junction_marks,
flips.joined_marks): short transpositions are found by fragment tilings, long ones by unit tilings over the weak junctions at their
breakpoints or the joins a scaffold made.

Two swaps whose spans are more than reach_bp apart share no sub-fragment pair whose price changes, so their scores add exactly:
plan_swaps accepts the best swap, then the best that neither overlaps an accepted span nor lies within reach_bp of it, and so on.  A
round that lowers logL all the same (the float32 re-centring of graal_edit_layout) is undone.
"""
import numpy as np

from . import spans as _sp
from .lib import SWAP_VALID
from .spans import _contigs, joined_marks, weak_junction_marks   # noqa: F401  (the marks are part of this module's interface too)

ROUND_COLUMNS = ("round", "swaps", "contigs", "logL", "kept")
COLUMNS = ("first", "mid", "last", "contig", "pos_first", "pos_mid", "pos_last", "frags_x", "frags_y", "score", "contacts", "status")


def tilings(soa, marks=None, max_units=8):
    """Yields (first, mid, last) int32 arrays: for span m = 2 .. max_units, split a = 1 .. m - 1 and offset = 0 .. m - 1 the swaps of a
    run of a units with the m - a units behind it that start offset, offset + m, ... units into each linear contig.  marks[f] true: a
    run may end after fragment f (None: after every fragment).  Spans of a set are disjoint; every pair of adjacent runs of at most
    max_units whole units together is a swap of exactly one set (a span that is its whole contig too); a set without swaps is left
    out."""
    contigs, units = _sp.unit_bounds(soa, marks)
    for m_units in range(2, int(max_units) + 1):
        for split in range(1, m_units):
            for offset in range(m_units):
                first, mid, last = [], [], []
                for m, u in zip(contigs, units):
                    a = np.arange(offset, len(u) - 1 - m_units + 1, m_units)
                    if len(a) == 0:
                        continue
                    first.append(m[u[a]]); mid.append(m[u[a + split] - 1]); last.append(m[u[a + m_units] - 1])
                if first:
                    yield tuple(np.concatenate(x).astype(np.int32) for x in (first, mid, last))


def plan_swaps(candidates, soa, reach_bp, min_score=0.0):
    """(first, mid, last, score) of the swaps to apply.  candidates: one (first, mid, last, score, status) tuple of arrays per scored
    call (or a single such tuple).  Taken: SWAP_VALID swaps with score > min_score, best first (ties: the lower (first, mid, last)); a
    swap whose span overlaps an accepted span of its contig, or whose bp interval lies within reach_bp of one, is skipped."""
    return _sp.plan(candidates, 5, SWAP_VALID, soa, reach_bp, min_score)


def swap_edit(soa, first, mid, last):
    """(cuts, joins) for graal_edit_layout that apply the disjoint swaps (X = first[k] .. mid[k], Y = behind mid[k] .. last[k]): a cut
    before X, between X and Y and behind Y where a neighbour exists, then along each contig the joins of consecutive pieces in the new
    order, Y in front of X, every piece entered through its head.  Several swaps may share a contig (adjacent ones too): the joins form
    a matching."""
    pos, idc = np.asarray(soa["pos"]), np.asarray(soa["id_c"])
    first, mid, last = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (first, mid, last))
    cuts, joins = [], []
    by_contig = {}
    for f, m_, l in zip(first, mid, last):
        by_contig.setdefault(int(idc[f]), []).append((int(pos[f]), int(pos[m_]), int(pos[l])))
    for c, spans in by_contig.items():
        m = np.nonzero(idc == c)[0]
        m = m[np.argsort(pos[m])]
        old, new, at = [], [], 0                 # pieces (first position, last position) in the current and in the new order
        for p0, pm, p1 in sorted(spans):
            if p0 < at or pm < p0 or p1 <= pm:
                raise ValueError("swap_edit: spans overlap or run backwards")
            if p0 > at:
                old.append((at, p0 - 1)); new.append((at, p0 - 1))
            old += [(p0, pm), (pm + 1, p1)]
            new += [(pm + 1, p1), (p0, pm)]
            at = p1 + 1
        if at < len(m):
            old.append((at, len(m) - 1)); new.append((at, len(m) - 1))
        cuts += [int(m[p1]) for _, p1 in old[:-1]]
        joins += [(2 * int(m[x[1]]) + 1, 2 * int(m[y[0]])) for x, y in zip(new[:-1], new[1:])]   # a piece's tail to the next one's head
    return np.array(sorted(cuts), dtype=np.int64), np.array(joins, dtype=np.int64).reshape(-1, 2)


def score_table(engine, soa, sets):
    """Every swap of the sets scored: a dict of numpy columns (COLUMNS), in the order of the sets."""
    pos, idc = np.asarray(soa["pos"]), np.asarray(soa["id_c"])
    cols = {k: [] for k in COLUMNS}
    for first, mid, last in sets:
        S, c, st = engine.block_swaps(first, mid, last)
        cols["first"].append(first); cols["mid"].append(mid); cols["last"].append(last); cols["contig"].append(idc[first])
        cols["pos_first"].append(pos[first]); cols["pos_mid"].append(pos[mid]); cols["pos_last"].append(pos[last])
        cols["frags_x"].append(pos[mid] - pos[first] + 1); cols["frags_y"].append(pos[last] - pos[mid])
        cols["score"].append(S); cols["contacts"].append(c); cols["status"].append(st)
    return {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}


def swap_rounds(sampler_or_engine, max_frags=8, junction_below=0.0, max_units=3, min_score=0.0, rounds=20, reach_bp=None, extra_marks=None):
    """Rounds of swaps on the engine's current layout.  A round scores the fragment tilings up to max_frags and the unit tilings (up to
    max_units units) over weak_junction_marks(junction_below) -- or'ed with extra_marks(soa) when given --, plans the swaps
    (plan_swaps), applies them in one edit_layout call and evaluates the layout in full.  A round that lowers logL is undone and the
    rounds stop there; they also stop when nothing is planned.  reach_bp: the window in bp (default: from the engine's parameters).
    Returns the record: a list of dicts with the keys ROUND_COLUMNS (and the cuts and joins of the edit), round 0 the layout as it came."""
    return _sp.run_rounds(sampler_or_engine, "swap", "block_swaps", tilings, plan_swaps, swap_edit, max_frags, junction_below, max_units,
                          min_score, rounds, reach_bp, extra_marks)


def write_swap_rounds_tsv(path, record):
    """swap_rounds' record as a TSV file with a header line; logL with 17 significant digits."""
    return _sp.write_rounds_tsv(path, record, ROUND_COLUMNS)


def write_swaps_tsv(path, table):
    """score_table's columns as a TSV file with a header line; scores with 17 significant digits (nan where there is none)."""
    return _sp.write_table_tsv(path, table, COLUMNS)
