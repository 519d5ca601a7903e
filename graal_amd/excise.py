"""Excisions: score cutting a run of fragments out of its contig (Engine.block_excisions) and excise the runs the data prefer on their own.

    tilings(soa, marks=None, max_units=3)                         -- disjoint span sets (first, last) that cover every short run once
    plan_excisions(candidates, soa, reach_bp, min_score=0.0)      -- the excisions of a round: best first, no two within reach of each other
    excise_edit(soa, first, last)                                 -- the cuts and joins that apply those excisions (graal_edit_layout)
    excise_rounds(sampler_or_engine, max_frags=3, ...)            -- the rounds; returns their record
    score_table(engine, soa, sets) / write_excisions_tsv, write_excise_rounds_tsv

A span is a run of fragments of one linear contig; the excised layout closes the gap behind it and leaves the run as a contig of its own:
the exact inverse of an insertion.  It is the repair for a short run that sits inside the wrong contig, or far from home in the right
one: the junction scores price the two junctions around it one at a time, and a cut at L | X R also severs every L x R pair, so both stay
positive although "L and R closed up, X on its own" is far more likely.  insert.insert_rounds afterwards places the freed pieces.
graal_block_excisions scores every span of a call alone, so the spans of a call must be disjoint: "every run of at most N units" is
N (N + 1) / 2 tilings.  A UNIT is a fragment (marks=None) or a maximal run between marked junctions (spans.weak_junction_marks,
spans.joined_marks).

Two excisions whose spans are more than reach_bp apart share no sub-fragment pair whose price changes, so their scores add exactly:
plan_excisions accepts the best span, then the best that neither overlaps an accepted one nor lies within reach_bp of it, and so on.  A
round that lowers logL all the same (the float32 re-centring of graal_edit_layout) is undone.
"""
import numpy as np

from . import flips as _flips
from . import spans as _sp
from .lib import EXCISE_VALID
from .spans import _contigs, joined_marks, weak_junction_marks   # noqa: F401  (the marks are part of this module's interface too)

ROUND_COLUMNS = ("round", "excisions", "contigs", "logL", "kept")
COLUMNS = ("first", "last", "contig", "pos_first", "pos_last", "frags", "score", "contacts", "status")


def tilings(soa, marks=None, max_units=3):
    """Yields (first, last) int32 arrays: for m = 1 .. max_units and offset = 0 .. m - 1 the spans of m consecutive units that start
    offset, offset + m, ... units into each linear contig.  marks[f] true: a span may end after fragment f (None: after every
    fragment).  Spans of a set are disjoint; every run of at most max_units whole units is a span of exactly one set; a span that is
    its whole contig is left out (nothing to cut), and so is a set without spans.  These are the flips' blocks: the same sets."""
    return _flips.tilings(soa, marks, max_units)


def plan_excisions(candidates, soa, reach_bp, min_score=0.0):
    """(first, last, score) of the excisions to apply.  candidates: one (first, last, score, status) tuple of arrays per scored call (or
    a single such tuple).  Taken: EXCISE_VALID spans with score > min_score, best first (ties: the lower (first, last)); a span that
    overlaps an accepted span of its contig, or whose bp interval lies within reach_bp of one, is skipped."""
    return _sp.plan(candidates, 4, EXCISE_VALID, soa, reach_bp, min_score)


def excise_edit(soa, first, last):
    """(cuts, joins) for graal_edit_layout that excise the disjoint spans (first[k] .. last[k]): a cut in front of and behind every span
    where a neighbour exists, then along each contig the joins of the consecutive pieces that stay, tail to head.  Several spans may
    share a contig (adjacent ones too): the pieces between them close up into one contig, every span is a contig of its own."""
    pos, idc = np.asarray(soa["pos"]), np.asarray(soa["id_c"])
    first, last = np.asarray(first, dtype=np.int64).reshape(-1), np.asarray(last, dtype=np.int64).reshape(-1)
    cuts, joins = [], []
    by_contig = {}
    for f, l in zip(first, last):
        by_contig.setdefault(int(idc[f]), []).append((int(pos[f]), int(pos[l])))
    for c, spans in by_contig.items():
        m = np.nonzero(idc == c)[0]
        m = m[np.argsort(pos[m])]
        pieces, at = [], 0                       # (first position, last position, excised) along the contig
        for p0, p1 in sorted(spans):
            if p0 < at or p1 < p0:
                raise ValueError("excise_edit: spans overlap or run backwards")
            if p0 > at:
                pieces.append((at, p0 - 1, False))
            pieces.append((p0, p1, True))
            at = p1 + 1
        if at < len(m):
            pieces.append((at, len(m) - 1, False))
        cuts += [int(m[p1]) for _, p1, _ in pieces[:-1]]
        kept = [(p0, p1) for p0, p1, out in pieces if not out]
        joins += [(2 * int(m[x[1]]) + 1, 2 * int(m[y[0]])) for x, y in zip(kept[:-1], kept[1:])]
    return np.array(sorted(cuts), dtype=np.int64), np.array(joins, dtype=np.int64).reshape(-1, 2)


def score_table(engine, soa, sets):
    """Every span of the sets scored: a dict of numpy columns (COLUMNS), in the order of the sets."""
    pos, idc = np.asarray(soa["pos"]), np.asarray(soa["id_c"])
    cols = {k: [] for k in COLUMNS}
    for first, last in sets:
        E, c, st = engine.block_excisions(first, last)
        cols["first"].append(first); cols["last"].append(last); cols["contig"].append(idc[first])
        cols["pos_first"].append(pos[first]); cols["pos_last"].append(pos[last]); cols["frags"].append(pos[last] - pos[first] + 1)
        cols["score"].append(E); cols["contacts"].append(c); cols["status"].append(st)
    return {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}


def excise_rounds(sampler_or_engine, max_frags=3, junction_below=0.0, max_units=3, min_score=0.0, rounds=20, reach_bp=None, extra_marks=None):
    """Rounds of excisions on the engine's current layout.  A round scores the fragment tilings up to max_frags and the unit tilings (up
    to max_units units) over weak_junction_marks(junction_below) -- or'ed with extra_marks(soa) when given --, plans the excisions
    (plan_excisions), applies them in one edit_layout call and evaluates the layout in full.  A round that lowers logL is undone and the
    rounds stop there; they also stop when nothing is planned.  reach_bp: the window in bp (default: from the engine's parameters).
    Returns the record: a list of dicts with the keys ROUND_COLUMNS (and the cuts and joins of the edit), round 0 the layout as it came."""
    return _sp.run_rounds(sampler_or_engine, "excision", "block_excisions", tilings, plan_excisions, excise_edit, max_frags, junction_below,
                          max_units, min_score, rounds, reach_bp, extra_marks)


def write_excise_rounds_tsv(path, record):
    """excise_rounds' record as a TSV file with a header line; logL with 17 significant digits."""
    return _sp.write_rounds_tsv(path, record, ROUND_COLUMNS)


def write_excisions_tsv(path, table):
    """score_table's columns as a TSV file with a header line; scores with 17 significant digits (nan where there is none)."""
    return _sp.write_table_tsv(path, table, COLUMNS)
