"""Inversions: score blocks of a layout flipped in place (Engine.block_flips) and flip those the data prefer.

    tilings(soa, marks=None, max_units=8)                         -- disjoint block sets (first, last) that cover every short run once
    weak_junction_marks(engine, below=0.0)                        -- marks from the junction scores
    joined_marks(soa_before, soa_now)                             -- marks at the boundaries of the pieces a scaffold joined
    plan_flips(candidates, soa, reach_bp, min_score=0.0)          -- the flips of a round: best first, no two within reach of each other
    flip_edit(soa, first, last)                                   -- the cuts and joins that flip those blocks (graal_edit_layout)
    flip_rounds(sampler_or_engine, max_frags=8, ...)              -- the rounds; returns their record
    score_table(engine, soa, sets) / write_flips_tsv, write_flip_rounds_tsv

A block is a run of fragments of one linear contig; graal_block_flips scores every block of a call alone, so the blocks of a call must
be disjoint: "every run of up to N units" is the N (N + 1) / 2 tilings (run length m, offset 0 .. m - 1).  A UNIT is a fragment
(marks=None) or a maximal run between marked junctions: short inversions are found by fragment tilings, long ones by unit tilings over
the weak junctions at their breakpoints (weak_junction_marks) or the joins a scaffold made (joined_marks).

Two flips whose blocks are more than reach_bp apart share no sub-fragment pair whose price changes, so their scores add exactly:
plan_flips accepts the best block, then the best block that neither overlaps an accepted one nor lies within reach_bp of it, and so
on.  A round that lowers logL all the same (the float32 re-centring of graal_edit_layout) is undone.
"""
import numpy as np

from . import scaffold as _sc   # noqa: F401  (part of this module's interface)
from . import spans as _sp
from .lib import FLIP_VALID
from .spans import _contigs, joined_marks, weak_junction_marks   # noqa: F401  (the marks are part of this module's interface)

ROUND_COLUMNS = ("round", "flips", "contigs", "logL", "kept")
COLUMNS = ("first", "last", "contig", "pos_first", "pos_last", "frags", "score", "contacts", "status")


def tilings(soa, marks=None, max_units=8):
    """Yields (first, last) int32 arrays: for m = 1 .. max_units and offset = 0 .. m - 1 the blocks of m consecutive units that start
    offset, offset + m, ... units into each linear contig.  marks[f] true: a block may end after fragment f (None: after every
    fragment).  Blocks of a set are disjoint; every run of at most max_units whole units is a block of exactly one set; a block that is
    its whole contig is left out, and so is a set without blocks."""
    contigs, units = _sp.unit_bounds(soa, marks)
    for m_units in range(1, int(max_units) + 1):
        for offset in range(m_units):
            first, last = [], []
            for m, u in zip(contigs, units):
                nu = len(u) - 1
                a = np.arange(offset, nu - m_units + 1, m_units)
                if len(a) == 0:
                    continue
                p0, p1 = u[a], u[a + m_units] - 1
                keep = ~((p0 == 0) & (p1 == len(m) - 1))
                first.append(m[p0[keep]]); last.append(m[p1[keep]])
            if first and sum(len(x) for x in first):
                yield np.concatenate(first).astype(np.int32), np.concatenate(last).astype(np.int32)


def plan_flips(candidates, soa, reach_bp, min_score=0.0):
    """(first, last, score) of the flips to apply.  candidates: one (first, last, score, status) tuple of arrays per scored call (or a
    single such tuple).  Taken: FLIP_VALID blocks with score > min_score, best first (ties: the lower (first, last)); a block that
    overlaps an accepted block of its contig, or whose bp interval lies within reach_bp of one, is skipped."""
    return _sp.plan(candidates, 4, FLIP_VALID, soa, reach_bp, min_score)


def flip_edit(soa, first, last):
    """(cuts, joins) for graal_edit_layout that reverse the disjoint blocks (first[k] .. last[k]) in place: a cut before and after every
    block where a neighbour exists, then along each contig the joins of consecutive pieces, a block entered through its tail and left
    through its head.  Several blocks may share a contig (adjacent ones too): the joins form a matching."""
    pos, idc = np.asarray(soa["pos"]), np.asarray(soa["id_c"])
    first, last = np.asarray(first, dtype=np.int64).reshape(-1), np.asarray(last, dtype=np.int64).reshape(-1)
    cuts, joins = [], []
    by_contig = {}
    for f, l in zip(first, last):
        by_contig.setdefault(int(idc[f]), []).append((int(pos[f]), int(pos[l])))
    for c, blocks in by_contig.items():
        m = np.nonzero(idc == c)[0]
        m = m[np.argsort(pos[m])]
        pieces, at = [], 0                       # (first position, last position, flipped) along the contig
        for p0, p1 in sorted(blocks):
            if p0 < at or p1 < p0:
                raise ValueError("flip_edit: blocks overlap or run backwards")
            if p0 > at:
                pieces.append((at, p0 - 1, False))
            pieces.append((p0, p1, True))
            at = p1 + 1
        if at < len(m):
            pieces.append((at, len(m) - 1, False))
        ends = [(2 * int(m[p1]) + 1, 2 * int(m[p0])) if flipped else (2 * int(m[p0]), 2 * int(m[p1]) + 1) for p0, p1, flipped in pieces]
        cuts += [int(m[p1]) for _, p1, _ in pieces[:-1]]
        joins += [(x[1], y[0]) for x, y in zip(ends[:-1], ends[1:])]   # leave a piece through its exit end, enter the next
    return np.array(sorted(cuts), dtype=np.int64), np.array(joins, dtype=np.int64).reshape(-1, 2)


def score_table(engine, soa, sets):
    """Every block of the sets scored: a dict of numpy columns (COLUMNS), in the order of the sets."""
    pos, idc = np.asarray(soa["pos"]), np.asarray(soa["id_c"])
    cols = {k: [] for k in COLUMNS}
    for first, last in sets:
        F, c, st = engine.block_flips(first, last)
        cols["first"].append(first); cols["last"].append(last); cols["contig"].append(idc[first])
        cols["pos_first"].append(pos[first]); cols["pos_last"].append(pos[last]); cols["frags"].append(pos[last] - pos[first] + 1)
        cols["score"].append(F); cols["contacts"].append(c); cols["status"].append(st)
    return {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}


def flip_rounds(sampler_or_engine, max_frags=8, junction_below=0.0, max_units=3, min_score=0.0, rounds=20, reach_bp=None, extra_marks=None):
    """Rounds of flips on the engine's current layout.  A round scores the fragment tilings up to max_frags and the unit tilings (up to
    max_units units) over weak_junction_marks(junction_below) -- or'ed with extra_marks(soa) when given --, plans the flips
    (plan_flips), applies them in one edit_layout call and evaluates the layout in full.  A round that lowers logL is undone and the
    rounds stop there; they also stop when nothing is planned.  reach_bp: the window in bp (default: from the engine's parameters).
    Returns the record: a list of dicts with the keys ROUND_COLUMNS (and the cuts and joins of the edit), round 0 the layout as it came."""
    return _sp.run_rounds(sampler_or_engine, "flip", "block_flips", tilings, plan_flips, flip_edit, max_frags, junction_below, max_units,
                          min_score, rounds, reach_bp, extra_marks)


def write_flip_rounds_tsv(path, record):
    """flip_rounds' record as a TSV file with a header line; logL with 17 significant digits."""
    return _sp.write_rounds_tsv(path, record, ROUND_COLUMNS)


def write_flips_tsv(path, table):
    """score_table's columns as a TSV file with a header line; scores with 17 significant digits (nan where there is none)."""
    return _sp.write_table_tsv(path, table, COLUMNS)
