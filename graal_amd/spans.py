"""What flips.py, swaps.py and excise.py share: a move of a span of one linear contig is named by its fragments (first, last for a flip
or an excision; first, mid, last for a swap), scored a disjoint set per call, planned best first and applied in rounds.

    unit_bounds(soa, marks=None)                                  -- the linear contigs and each one's unit boundaries
    weak_junction_marks(engine, below=0.0)                        -- marks from the junction scores
    joined_marks(soa_before, soa_now)                             -- marks at the boundaries of the pieces a scaffold joined
    stack(candidates, width) / plan(candidates, width, valid, soa, reach_bp, min_score)
    run_rounds(sampler_or_engine, who, call, tilings, plan, edit, ...)
    write_rounds_tsv(path, record, columns) / write_table_tsv(path, table, columns)

A UNIT is a fragment (marks=None) or a maximal run between marked junctions.  Two moves whose spans are more than reach_bp apart share
no sub-fragment pair whose price changes, so their scores add exactly: that is what plan relies on.
"""
import numpy as np

from . import scaffold as _sc
from .lib import JUNCTION_VALID


def _contigs(soa):
    """The linear contigs as arrays of fragments in position order, in label order."""
    idc, pos, circ = (np.asarray(soa[k]) for k in ("id_c", "pos", "circ"))
    order = np.lexsort((pos, idc))
    cut = np.nonzero(np.diff(idc[order]))[0] + 1
    return [m for m in np.split(order, cut) if len(m) and circ[m[0]] != 1]


def unit_bounds(soa, marks=None):
    """(contigs, units): _contigs(soa) and, per contig, the position of each unit's first fragment followed by the contig's length.
    marks[f] true: a unit may end after fragment f (None: after every fragment)."""
    contigs = _contigs(soa)
    units = []
    for m in contigs:
        if marks is None:
            starts = np.arange(len(m))
        else:
            mk = np.asarray(marks, dtype=bool)[m[:-1]]
            starts = np.concatenate([[0], np.nonzero(mk)[0] + 1])
        units.append(np.append(starts, len(m)))
    return contigs, units


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


def stack(candidates, width):
    """The candidates' columns concatenated: width - 2 int64 fragment columns, the float64 scores, the uint8 status bytes.  candidates:
    one tuple of `width` arrays per scored call, or a single such tuple."""
    if isinstance(candidates, tuple) and len(candidates) == width and not isinstance(candidates[0], tuple):
        candidates = [candidates]
    types = (np.int64,) * (width - 2) + (np.float64, np.uint8)
    cols = [[np.asarray(c[i]).reshape(-1) for c in candidates] for i in range(width)]
    if not cols[0]:
        return tuple(np.zeros(0, t) for t in types)
    return tuple(np.concatenate(cols[i]).astype(t) for i, t in enumerate(types))


def plan(candidates, width, valid, soa, reach_bp, min_score=0.0):
    """The moves to apply: their fragment columns and scores.  Taken: candidates of status `valid` with score > min_score, best first
    (ties: the lower fragment columns, the first column first); a span that overlaps an accepted span of its contig, or whose bp
    interval lies within reach_bp of one, is skipped."""
    *frags, score, st = stack(candidates, width)
    with np.errstate(invalid="ignore"):
        ok = (st == valid) & (score > float(min_score))
    frags, score = [c[ok] for c in frags], score[ok]
    idc, start, ln = (np.asarray(soa[k], dtype=np.int64) for k in ("id_c", "start_bp", "len_bp"))
    order = np.lexsort(tuple(frags[::-1]) + (-score,))
    taken = {}                                   # contig -> accepted (s0, e1)
    out = []
    for i in order:
        f, l = int(frags[0][i]), int(frags[-1][i])
        s0, e1 = int(start[f]), int(start[l] + ln[l])
        mine = taken.setdefault(int(idc[f]), [])
        if any(s0 - b <= reach_bp and a - e1 <= reach_bp for a, b in mine):   # (overlap: both gaps negative)
            continue
        mine.append((s0, e1))
        out.append(i)
    out = np.array(out, dtype=np.int64)
    return tuple(c[out] for c in frags) + (score[out],)


def run_rounds(sampler_or_engine, who, call, tilings, plan_moves, edit, max_frags, junction_below, max_units, min_score, rounds, reach_bp,
               extra_marks):
    """Rounds of moves on the engine's current layout.  A round scores (the Engine method `call`) the fragment tilings up to max_frags
    and the unit tilings (up to max_units units) over weak_junction_marks(junction_below) -- or'ed with extra_marks(soa) when given --,
    plans the moves, applies them in one edit_layout call and evaluates the layout in full.  A round that lowers logL is undone and the
    rounds stop there; they also stop when nothing is planned.  Returns the record: a list of dicts, the number of moves under the key
    who + "s", round 0 the layout as it came."""
    obj = sampler_or_engine
    e = _sc._engine(obj)
    if reach_bp is None:
        par = getattr(e, "param", None)
        if par is None:
            raise ValueError(who + "_rounds: reach_bp is needed (the engine's parameters were not set through this Engine object)")
        # (the engine's reach_bp(h) in csrc/graal_hip.hip, restated: ceil(d_max * 1000) + 1000 from the float32 d_max.  The planner
        # only needs a bound that is not smaller: a larger one keeps accepted moves further apart, never closer.)
        reach_bp = int(np.ceil(np.float64(np.float32(par[5])) * 1000.0)) + 1000
    logl, nc = _sc._evaluate(e)
    record = [{"round": 0, who + "s": 0, "cuts": 0, "joins": 0, "contigs": nc, "logL": logl, "kept": 1}]
    for r in range(1, int(rounds) + 1):
        before = e.download_frags()
        marks = weak_junction_marks(e, junction_below)
        if extra_marks is not None:
            marks = marks | np.asarray(extra_marks(before), dtype=bool)
        cands = []
        for sets in (tilings(before, None, max_frags), tilings(before, marks, max_units) if marks.any() else ()):
            for frags in sets:
                q, _, st = getattr(e, call)(*frags)
                cands.append(tuple(frags) + (q, st))
        *frags, _ = plan_moves(cands, before, reach_bp, min_score)
        if len(frags[0]) == 0:
            break
        cuts, joins = edit(before, *frags)
        _sc._edit(obj, e, cuts, joins)
        new_logl, nc = _sc._evaluate(e)
        row = {"round": r, who + "s": int(len(frags[0])), "cuts": int(len(cuts)), "joins": int(len(joins)), "contigs": nc, "logL": new_logl,
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


def write_rounds_tsv(path, record, columns):
    """A rounds record as a TSV file with a header line (columns: round, moves, contigs, logL, kept); logL with 17 significant digits."""
    with open(path, "w") as fh:
        fh.write("\t".join(columns) + "\n")
        for row in record:
            fh.write("\t".join([str(int(row[c])) for c in columns[:3]] + [repr(float(row["logL"])), str(int(row["kept"]))]) + "\n")
    return len(record)


def write_table_tsv(path, table, columns):
    """A score table's columns as a TSV file with a header line; scores with 17 significant digits (nan where there is none)."""
    n = len(table["first"])
    with open(path, "w") as fh:
        fh.write("\t".join(columns) + "\n")
        for i in range(n):
            fh.write("\t".join(repr(float(table[c][i])) if c == "score" else str(int(table[c][i])) for c in columns) + "\n")
    return n
