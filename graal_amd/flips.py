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

from . import scaffold as _sc
from .lib import FLIP_VALID, JUNCTION_VALID

ROUND_COLUMNS = ("round", "flips", "contigs", "logL", "kept")
COLUMNS = ("first", "last", "contig", "pos_first", "pos_last", "frags", "score", "contacts", "status")


def _contigs(soa):
    """The linear contigs as arrays of fragments in position order, in label order."""
    idc, pos, circ = (np.asarray(soa[k]) for k in ("id_c", "pos", "circ"))
    order = np.lexsort((pos, idc))
    cut = np.nonzero(np.diff(idc[order]))[0] + 1
    return [m for m in np.split(order, cut) if len(m) and circ[m[0]] != 1]


def tilings(soa, marks=None, max_units=8):
    """Yields (first, last) int32 arrays: for m = 1 .. max_units and offset = 0 .. m - 1 the blocks of m consecutive units that start
    offset, offset + m, ... units into each linear contig.  marks[f] true: a block may end after fragment f (None: after every
    fragment).  Blocks of a set are disjoint; every run of at most max_units whole units is a block of exactly one set; a block that is
    its whole contig is left out, and so is a set without blocks."""
    contigs = _contigs(soa)
    units = []                                   # per contig: the position of each unit's first fragment, and the contig's length
    for m in contigs:
        if marks is None:
            starts = np.arange(len(m))
        else:
            mk = np.asarray(marks, dtype=bool)[m[:-1]]
            starts = np.concatenate([[0], np.nonzero(mk)[0] + 1])
        units.append(np.append(starts, len(m)))
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


def weak_junction_marks(engine, below=0.0):
    """marks[f] true where the junction after f is scored (JUNCTION_VALID) and its score is below `below`."""
    J, st = engine.junction_scores()
    with np.errstate(invalid="ignore"):
        return (st == JUNCTION_VALID) & (J < float(below))


def joined_marks(soa_before, soa_now):
    """marks[f] true for a junction (f, next[f]) of soa_now unless the two fragments were neighbours in the same relative orientation in
    soa_before: the boundaries of the pieces joined since then."""
    nx = np.asarray(soa_now["next"])
    n = len(nx)
    f = np.nonzero(nx >= 0)[0]
    g = nx[f]
    nb, pb = np.asarray(soa_before["next"]), np.asarray(soa_before["prev"])
    same_f = np.asarray(soa_before["ori"])[f] == np.asarray(soa_now["ori"])[f]
    same_g = np.asarray(soa_before["ori"])[g] == np.asarray(soa_now["ori"])[g]
    kept = ((nb[f] == g) & same_f & same_g) | ((pb[f] == g) & ~same_f & ~same_g)
    marks = np.zeros(n, dtype=bool)
    marks[f[~kept]] = True
    return marks


def _stack(candidates):
    if isinstance(candidates, tuple) and len(candidates) == 4 and not isinstance(candidates[0], tuple):
        candidates = [candidates]
    cols = [[np.asarray(c[i]).reshape(-1) for c in candidates] for i in range(4)]
    if not cols[0]:
        return (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.uint8))
    return (np.concatenate(cols[0]).astype(np.int64), np.concatenate(cols[1]).astype(np.int64), np.concatenate(cols[2]).astype(np.float64),
            np.concatenate(cols[3]).astype(np.uint8))


def plan_flips(candidates, soa, reach_bp, min_score=0.0):
    """(first, last, score) of the flips to apply.  candidates: one (first, last, score, status) tuple of arrays per scored call (or a
    single such tuple).  Taken: FLIP_VALID blocks with score > min_score, best first (ties: the lower (first, last)); a block that
    overlaps an accepted block of its contig, or whose bp interval lies within reach_bp of one, is skipped."""
    first, last, score, st = _stack(candidates)
    with np.errstate(invalid="ignore"):
        ok = (st == FLIP_VALID) & (score > float(min_score))
    first, last, score = first[ok], last[ok], score[ok]
    idc, start, ln = (np.asarray(soa[k], dtype=np.int64) for k in ("id_c", "start_bp", "len_bp"))
    order = np.lexsort((last, first, -score))
    taken = {}                                   # contig -> accepted (s0, e1)
    out = []
    for i in order:
        f, l = int(first[i]), int(last[i])
        s0, e1 = int(start[f]), int(start[l] + ln[l])
        mine = taken.setdefault(int(idc[f]), [])
        if any(s0 - b <= reach_bp and a - e1 <= reach_bp for a, b in mine):   # (overlap: both gaps negative)
            continue
        mine.append((s0, e1))
        out.append((f, l, float(score[i])))
    if not out:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    a, b, c = zip(*out)
    return np.array(a, np.int64), np.array(b, np.int64), np.array(c, np.float64)


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
    obj = sampler_or_engine
    e = _sc._engine(obj)
    if reach_bp is None:
        par = getattr(e, "param", None)
        if par is None:
            raise ValueError("flip_rounds: reach_bp is needed (the engine's parameters were not set through this Engine object)")
        # (the engine's reach_bp(h) in csrc/graal_hip.hip, restated: ceil(d_max * 1000) + 1000 from the float32 d_max.  The planner
        # only needs a bound that is not smaller: a larger one keeps accepted flips further apart, never closer.)
        reach_bp = int(np.ceil(np.float64(np.float32(par[5])) * 1000.0)) + 1000
    logl, nc = _sc._evaluate(e)
    record = [{"round": 0, "flips": 0, "cuts": 0, "joins": 0, "contigs": nc, "logL": logl, "kept": 1}]
    for r in range(1, int(rounds) + 1):
        before = e.download_frags()
        marks = weak_junction_marks(e, junction_below)
        if extra_marks is not None:
            marks = marks | np.asarray(extra_marks(before), dtype=bool)
        cands = []
        for sets in (tilings(before, None, max_frags), tilings(before, marks, max_units) if marks.any() else ()):
            for first, last in sets:
                F, _, st = e.block_flips(first, last)
                cands.append((first, last, F, st))
        first, last, _ = plan_flips(cands, before, reach_bp, min_score)
        if len(first) == 0:
            break
        cuts, joins = flip_edit(before, first, last)
        _sc._edit(obj, e, cuts, joins)
        new_logl, nc = _sc._evaluate(e)
        row = {"round": r, "flips": int(len(first)), "cuts": int(len(cuts)), "joins": int(len(joins)), "contigs": nc, "logL": new_logl,
               "kept": 1}
        if not new_logl >= logl:       # (NaN included)
            row["kept"] = 0
            record.append(row)
            _sc._restore(obj, e, before)
            _sc._evaluate(e)
            break
        record.append(row)
        logl = new_logl
    return record


def write_flip_rounds_tsv(path, record):
    """flip_rounds' record as a TSV file with a header line; logL with 17 significant digits."""
    with open(path, "w") as fh:
        fh.write("\t".join(ROUND_COLUMNS) + "\n")
        for row in record:
            fh.write("\t".join([str(int(row[c])) for c in ROUND_COLUMNS[:3]] + [repr(float(row["logL"])), str(int(row["kept"]))]) + "\n")
    return len(record)


def write_flips_tsv(path, table):
    """score_table's columns as a TSV file with a header line; scores with 17 significant digits (nan where there is none)."""
    n = len(table["first"])
    with open(path, "w") as fh:
        fh.write("\t".join(COLUMNS) + "\n")
        for i in range(n):
            fh.write("\t".join(repr(float(table[c][i])) if c == "score" else str(int(table[c][i])) for c in COLUMNS) + "\n")
    return n
