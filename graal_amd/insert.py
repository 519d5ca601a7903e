"""Insertions: how strongly the data support putting a small contig into a junction of another contig (graal_insertions, HIP on the GPU),
and the planning of a round of them for graal_amd.scaffold.

A piece is a linear contig of 1 .. max_piece_frags fragments.  For a piece P, a junction f -> g = next[f] of another linear contig T and
rev in {0, 1}, score = logL(the layout with T cut between f and g and P put in between) - logL(layout) in the engine's exact arithmetic:
P's head next to f (rev 0) or its tail next to f (rev 1).  Only candidates with at least one contact between P and T inside the contact
model's window (d_max) in the inserted layout are listed: any other would score only its negative expected mass.

    insertion_table(sampler_or_engine, max_piece_frags=1)   -- the listed candidates as a dict of columns (see COLUMNS)
    fitting_insertion_table(sampler_or_engine, max_piece_frags)  -- the same at the largest piece size <= max_piece_frags that fits the
                                                            device budget: (table or None, that size or None)
    best_insertions(table)                                  -- per piece its best (after, rev), per junction its best piece (row indices)
    mutual_insertions(table)                                -- the rows that are both their piece's best and their junction's best
    plan_insertions(table, soa, min_score=0.0)              -- one round: the kept insertions, as cuts and joins for graal_edit_layout
    write_insertions_tsv(path, table)                       -- one tab-separated row per candidate, with a header line
"""
import numpy as np

from .lib import Engine, GraalError, INSERT_NONFINITE, INSERT_VALID

COLUMNS = ("piece_contig", "piece", "piece_frags", "target_contig", "after", "next", "rev", "contacts", "score")
STATUS_NAMES = {INSERT_VALID: "valid", INSERT_NONFINITE: "nonfinite"}


def _engine(obj):
    if isinstance(obj, Engine):
        return obj
    e = getattr(obj, "engine", None)
    if isinstance(e, Engine):
        return e
    raise TypeError("insertion_table takes a graal_amd Engine or a sampler that holds one (.engine), not %r" % type(obj).__name__)


def table_from(soa, piece, after, rev, contacts, score):
    """The insertion table of layout `soa` (the engine's fragment fields) from graal_insertions' columns (score NaN: no score)."""
    p = np.asarray(piece, dtype=np.int64)
    f = np.asarray(after, dtype=np.int64)
    idc = np.asarray(soa["id_c"], dtype=np.int64)
    return {"piece_contig": idc[p], "piece": p, "piece_frags": np.asarray(soa["l_cont"], dtype=np.int64)[p], "target_contig": idc[f],
            "after": f, "next": np.asarray(soa["next"], dtype=np.int64)[f], "rev": np.asarray(rev, dtype=np.int64),
            "contacts": np.asarray(contacts, dtype=np.int64), "score": np.asarray(score, dtype=np.float64)}


def insertion_table(sampler_or_engine, max_piece_frags=1):
    """The insertions of the engine's current layout with pieces of <= max_piece_frags fragments: a dict of numpy columns COLUMNS,
    sorted by (after, piece, rev)."""
    e = _engine(sampler_or_engine)
    p, f, r, score, c, _ = e.insertions(max_piece_frags)
    return table_from(e.download_frags(), p, f, r, c, score)


def fitting_insertion_table(sampler_or_engine, max_piece_frags):
    """insertion_table at max_piece_frags, or at the largest smaller piece size whose candidate table fits the device budget
    (GRAAL_LINKS_MAX_BYTES), with a message; (None, None) when not even pieces of one fragment fit.  Returns (table, the size used)."""
    for m in range(int(max_piece_frags), 0, -1):
        try:
            return insertion_table(sampler_or_engine, m), m
        except GraalError as err:
            if "GRAAL_LINKS_MAX_BYTES" not in str(err):
                raise
            print("graal_amd.insert: the insertions of pieces of <= %d fragments are over the device budget; %s" %
                  (m, "trying %d" % (m - 1) if m > 1 else "no table"))
    return None, None


def _best(key, other, score):
    """Per distinct key, the row with the highest score (ties: the lower `other`); rows without a finite score take no part."""
    ok = np.nonzero(np.isfinite(score))[0]
    order = ok[np.lexsort((other[ok], -score[ok], key[ok]))]
    first = np.concatenate([[True], key[order][1:] != key[order][:-1]]) if len(order) else np.zeros(0, bool)
    return dict(zip(key[order][first].tolist(), order[first].tolist()))


def best_insertions(table):
    """(by_piece, by_junction): {piece: row} with the piece's best (after, rev) -- ties: the lower (after, rev) -- and {after: row} with
    the junction's best piece -- ties: the lower (piece, rev).  Rows without a finite score take no part."""
    p, f, r = (np.asarray(table[k], dtype=np.int64) for k in ("piece", "after", "rev"))
    score = np.asarray(table["score"], dtype=np.float64)
    return _best(p, 2 * f + r, score), _best(f, 2 * p + r, score)


def mutual_insertions(table):
    """The row indices (increasing) that are their piece's best insertion and their junction's best piece."""
    by_piece, by_junction = best_insertions(table)
    f = np.asarray(table["after"], dtype=np.int64)
    return np.array(sorted(i for i in by_piece.values() if by_junction.get(int(f[i])) == i), dtype=np.int64)


def plan_insertions(table, soa, min_score=0.0):
    """One round of insertions from `table` (insertion_table's dict of layout `soa`): the mutual pairs with score > min_score.  A piece
    moved in the round is not a target in it: when a kept insertion moves a piece another kept insertion targets, the one with the higher
    score stays (ties: the lower (after, piece)).  Returns (cuts, joins, rows): the fragments to cut after, the (end, end) joins for
    graal_edit_layout -- (2f + 1, the piece's end facing f) and (its other end, 2 next[f]) per insertion, end = 2 * fragment + side --
    and the kept row indices in (after, piece) order."""
    rows = mutual_insertions(table)
    score = np.asarray(table["score"], dtype=np.float64)
    rows = rows[score[rows] > float(min_score)] if len(rows) else rows
    f, p = np.asarray(table["after"], dtype=np.int64), np.asarray(table["piece"], dtype=np.int64)
    pc, tc = np.asarray(table["piece_contig"], dtype=np.int64), np.asarray(table["target_contig"], dtype=np.int64)
    moved, targeted, kept = set(), set(), []
    for i in sorted(rows.tolist(), key=lambda i: (-score[i], f[i], p[i])):
        if int(pc[i]) in targeted or int(tc[i]) in moved:
            continue
        kept.append(i)
        moved.add(int(pc[i]))
        targeted.add(int(tc[i]))
    kept = np.array(sorted(kept, key=lambda i: (f[i], p[i])), dtype=np.int64)
    idc, pos, lc = (np.asarray(soa[k], dtype=np.int64) for k in ("id_c", "pos", "l_cont"))
    cuts, joins = [], []
    for i in kept.tolist():
        members = np.nonzero(idc == pc[i])[0]
        head, tail = int(p[i]), int(members[np.argmax(pos[members])]) if lc[p[i]] > 1 else int(p[i])
        near, far = (2 * head, 2 * tail + 1) if table["rev"][i] == 0 else (2 * tail + 1, 2 * head)
        cuts.append(int(f[i]))
        joins.append((2 * int(f[i]) + 1, near))
        joins.append((far, 2 * int(table["next"][i])))
    return np.asarray(cuts, dtype=np.int64), np.asarray(joins, dtype=np.int64).reshape(-1, 2), kept


def write_insertions_tsv(path, table):
    """Write `table` (insertion_table's dict) as a TSV file with a header line; scores with 17 significant digits, NaN as 'nan'."""
    n = len(table["score"])
    with open(path, "w") as fh:
        fh.write("\t".join(COLUMNS) + "\n")
        for i in range(n):
            row = [str(int(table[c][i])) for c in COLUMNS[:-1]]
            s = float(table["score"][i])
            row.append("nan" if not np.isfinite(s) else repr(s))
            fh.write("\t".join(row) + "\n")
    return n
