"""Greedy scaffolding and polishing of a layout on the GPU: join mutual-best contig ends, cut the junctions the data reject, round by round.

    scaffold(sampler_or_engine, rounds=50, min_score=0.0, min_frags=1, cut_below=None,
             insert_max_frags=None, insert_min_score=0.0,
             flip_max_frags=None, flip_min_score=0.0,
             swap_max_frags=None, swap_min_score=0.0, close_rings_min_score=None)     -- the rounds; returns their record
    break_cycles(ea, eb, score, contig_of_end)                                            -- drop the weakest join of every cycle
    write_scaffold_tsv(path, record)                                                      -- one tab-separated row per round

A round:
  1. (first round only, when cut_below is set) cut every junction whose junction score (graal_junction_scores) is below cut_below, in
     one graal_edit_layout call.  Only the first round cuts: a cut frees two ends, which the same round can rejoin elsewhere, and a join
     made later is a mutual-best link with a positive score, which no later round has reason to undo; cutting every round would let a
     weak but true join flip back and forth.  The cuts come before the links are scored, so the freed ends take part in this round's joins;
  2. the mutual-best links (graal_end_links_best) with score > min_score;
  3. every cycle of contigs those joins would close is broken at its weakest join (lowest score; ties: the larger (end_a, end_b));
  4. the joins in one graal_edit_layout call;
  5. a full evaluation (relabel, eval_full).
With insert_max_frags set, a round whose step 2 finds no join runs an insertion step instead (graal_amd.insert.plan_insertions: the
mutual-best insertions of pieces of <= insert_max_frags fragments scoring above insert_min_score, each a cut and two joins, in one
graal_edit_layout call), then the full evaluation; its row counts those cuts and joins.  When the insertion table of pieces that
large is over the device budget, the step uses the largest smaller piece size that fits (down to 1, else it is skipped).
Scaffolding stops when a round has no join (and no insertion) left.  Joins are scored one at a time and combined joins are not additive: a round that lowers
logL is undone (the layout from before the round is uploaded again) and scaffolding stops there.
With flip_max_frags set, once a round finds no join, cut or insertion left (not when `rounds` ran out first, and not behind a round that
was undone), graal_amd.flips.flip_rounds runs over the result with its own default number of rounds (fragment runs of up to
flip_max_frags fragments scoring above flip_min_score; its unit tilings are delimited by the weak junctions and by the joins made since
the layout scaffold() started from: a piece joined the wrong way round is one unit).  Its rounds follow in the record, numbered on, their
cuts and joins those of the flips' edits.
With swap_max_frags set, under the same condition and BEFORE the flip rounds, graal_amd.swaps.swap_rounds runs over the result (pairs
of adjacent runs of up to swap_max_frags fragments together scoring above swap_min_score, and unit tilings over the same marks): a run
that sits a few places from where it belongs is moved there, so that a moved run that is also inverted is at its place when the flips
look at it.  The joins those rounds made are marks of the flip rounds, as scaffold()'s own are.
With close_rings_min_score set, under the same condition and BEFORE the swap and flip rounds, graal_amd.rings.close_rings runs over the
result: step 3 opens every cycle of contigs, so a circular replicon ends the rounds as a linear chain, and this closes the chains whose
ring score (graal_ring_scores) is above close_rings_min_score, all at once (their scores add exactly).  Its row follows in the record:
joins = the contigs closed, kept 0 when logL did not rise by the summed scores and the closures were undone.
"""
import numpy as np

from .lib import Engine, JUNCTION_VALID, Q_SCALE

COLUMNS = ("round", "cuts", "joins", "contigs", "logL", "kept")


def _engine(obj):
    if isinstance(obj, Engine):
        return obj
    e = getattr(obj, "engine", None)
    if isinstance(e, Engine):
        return e
    raise TypeError("scaffold takes a graal_amd Engine or a sampler that holds one (.engine), not %r" % type(obj).__name__)


def break_cycles(ea, eb, score, contig_of_end):
    """A boolean mask over the joins (ea[i], eb[i], score[i]): False for the weakest join of every cycle of contigs the joins close
    (contig_of_end(end) -> contig label).  The joins are a matching of ends, so every contig has at most two joins and a component is a
    chain or a cycle: adding the joins strongest first (ties: the lower (end_a, end_b) first), the join that closes a cycle is its weakest."""
    ea, eb = np.asarray(ea, dtype=np.int64), np.asarray(eb, dtype=np.int64)
    score = np.asarray(score, dtype=np.float64)
    lo, hi = np.minimum(ea, eb), np.maximum(ea, eb)
    order = np.lexsort((hi, lo, -score))
    parent = {}

    def root(c):
        while parent.get(c, c) != c:
            parent[c] = parent.get(parent[c], parent[c])
            c = parent[c]
        return c

    keep = np.ones(len(ea), dtype=bool)
    for i in order:
        a, b = root(int(contig_of_end(int(ea[i])))), root(int(contig_of_end(int(eb[i]))))
        if a == b:
            keep[i] = False
        else:
            parent[a] = b
    return keep


def _edit(obj, e, cuts, joins):
    if hasattr(obj, "edit_layout") and not isinstance(obj, Engine):
        return obj.edit_layout(cuts, joins)
    return e.edit_layout(cuts, joins)


def _restore(obj, e, state):
    e.upload_frags(state)
    if not isinstance(obj, Engine) and hasattr(obj, "likelihood_t"):
        obj.likelihood_t = None


def _evaluate(e):
    e.relabel_contigs()
    return e.eval_full(), len(np.unique(e.download_frags()["id_c"]))


def plan_joins(mutual, min_score, contig_of_end):
    """The joins of a round from the mutual-best links (end_a, end_b, q): those with score > min_score, cycles broken.  (ea, eb, score)."""
    a, b, q = (np.asarray(x) for x in mutual)
    score = q.astype(np.float64) / Q_SCALE
    ok = score > float(min_score)
    a, b, score = a[ok], b[ok], score[ok]
    keep = break_cycles(a, b, score, contig_of_end)
    return a[keep], b[keep], score[keep]


def scaffold(sampler_or_engine, rounds=50, min_score=0.0, min_frags=1, cut_below=None, insert_max_frags=None, insert_min_score=0.0,
             flip_max_frags=None, flip_min_score=0.0, swap_max_frags=None, swap_min_score=0.0, close_rings_min_score=None):
    """Scaffold (and with cut_below, polish; with insert_max_frags, insert pieces) the engine's current layout; see the module's
    docstring.  Returns the record: a list of dicts with the keys COLUMNS, round 0 the layout as it came (kept 0 marks a round that was
    undone)."""
    obj = sampler_or_engine
    e = _engine(obj)
    start = e.download_frags() if flip_max_frags is not None or swap_max_frags is not None else None
    logl, nc = _evaluate(e)
    record = [{"round": 0, "cuts": 0, "joins": 0, "contigs": nc, "logL": logl, "kept": 1}]
    settled = False                # a round found no join, cut or insertion left
    for r in range(1, int(rounds) + 1):
        before = e.download_frags()
        cuts = np.zeros(0, dtype=np.int64)
        if cut_below is not None and r == 1:
            J, st = e.junction_scores()
            cuts = np.nonzero((st == JUNCTION_VALID) & (J < float(cut_below)))[0]
            if len(cuts):
                _edit(obj, e, cuts, np.zeros((0, 2), dtype=np.int64))
        idc = e.download_frags()["id_c"] if len(cuts) else before["id_c"]
        _, _, mutual = e.end_links_best(min_frags)
        a, b, _ = plan_joins(mutual, min_score, lambda end: idc[end >> 1])
        icuts, ijoins = np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.int64)
        if len(a) == 0 and insert_max_frags is not None:
            from . import insert
            soa = e.download_frags() if len(cuts) else before
            table, insert_max_frags = insert.fitting_insertion_table(e, insert_max_frags)
            if table is not None:
                icuts, ijoins, _ = insert.plan_insertions(table, soa, insert_min_score)
            if len(icuts):
                _edit(obj, e, icuts, ijoins)
        if len(a) == 0 and len(cuts) == 0 and len(icuts) == 0:
            settled = True
            break
        if len(a):
            _edit(obj, e, [], np.stack([a, b], axis=1))
        new_logl, nc = _evaluate(e)
        row = {"round": r, "cuts": int(len(cuts) + len(icuts)), "joins": int(len(a) + len(ijoins)), "contigs": nc, "logL": new_logl,
               "kept": 1}
        if not new_logl >= logl:       # (NaN included)
            row["kept"] = 0
            record.append(row)
            _restore(obj, e, before)
            _evaluate(e)
            break
        record.append(row)
        logl = new_logl
        if len(a) == 0 and len(icuts) == 0:
            settled = True             # (only cuts: no join and no insertion was on offer behind them)
            break
    if close_rings_min_score is not None and settled:
        from . import rings
        rec = rings.close_rings(obj, min_score=close_rings_min_score)
        record.append({"round": record[-1]["round"] + 1, "cuts": 0, "joins": rec["closed"], "contigs": rec["contigs"],
                       "logL": rec["logL"], "kept": rec["kept"]})
    if swap_max_frags is not None and settled:
        from . import flips, swaps
        last = record[-1]["round"]
        for row in swaps.swap_rounds(obj, max_frags=swap_max_frags, min_score=swap_min_score,
                                     extra_marks=lambda now: flips.joined_marks(start, now))[1:]:
            record.append({"round": last + row["round"], "cuts": row["cuts"], "joins": row["joins"], "contigs": row["contigs"],
                           "logL": row["logL"], "kept": row["kept"]})
    if flip_max_frags is not None and settled:
        from . import flips
        last = record[-1]["round"]
        for row in flips.flip_rounds(obj, max_frags=flip_max_frags, min_score=flip_min_score,
                                     extra_marks=lambda now: flips.joined_marks(start, now))[1:]:
            record.append({"round": last + row["round"], "cuts": row["cuts"], "joins": row["joins"], "contigs": row["contigs"],
                           "logL": row["logL"], "kept": row["kept"]})
    return record


def write_scaffold_tsv(path, record):
    """Write scaffold()'s record as a TSV file with a header line; logL with 17 significant digits."""
    with open(path, "w") as fh:
        fh.write("\t".join(COLUMNS) + "\n")
        for row in record:
            fh.write("\t".join([str(int(row[c])) for c in COLUMNS[:4]] + [repr(float(row["logL"])), str(int(row["kept"]))]) + "\n")
    return len(record)
