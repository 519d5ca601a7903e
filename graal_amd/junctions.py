"""Junction scores: how strongly the data support each join of a layout (graal_junction_scores, HIP on the GPU).

For a fragment f in a linear contig with a successor, J = logL(layout) - logL(the layout cut between f and its successor), in the
engine's exact arithmetic: only the sub-fragment pairs that straddle the cut change, from their cis price to their trans price.  A
positive J means the data prefer the join; a join with J <= 0 is one the data would rather see cut (a candidate misjoin).

    junction_table(sampler_or_engine)   -- the junctions in contig order, as a dict of columns (see COLUMNS)
    write_junctions_tsv(path, table)    -- one tab-separated row per junction, with a header line

Junction support (graal_junction_bootstrap): a Poisson bootstrap of the read pairs -- every contact's count redrawn as Poisson(count), n_rep
times, all replicates in one GPU call -- says how sure a score's sign is: `support` is the fraction of the replicates in which the
junction still scores above the threshold.

    support_table(sampler_or_engine, seed, n_rep, threshold=0.0)   -- junction_table's columns plus SUPPORT_COLUMNS[len(COLUMNS):]
    write_support_tsv(path, table)                                 -- the same as a TSV file
"""
import numpy as np

from .lib import Engine, JUNCTION_CIRCULAR, JUNCTION_END, JUNCTION_NONFINITE, JUNCTION_VALID

COLUMNS = ("contig", "position", "left_frag", "right_frag", "left_ori", "right_ori", "join_bp", "score")
SUPPORT_COLUMNS = COLUMNS + ("support", "boot_mean", "boot_min", "boot_max")
STATUS_NAMES = {JUNCTION_VALID: "valid", JUNCTION_END: "contig_end", JUNCTION_CIRCULAR: "circular", JUNCTION_NONFINITE: "nonfinite"}


def _engine(obj):
    if isinstance(obj, Engine):
        return obj
    e = getattr(obj, "engine", None)
    if isinstance(e, Engine):
        return e
    raise TypeError("junction_table takes a graal_amd Engine or a sampler that holds one (.engine), not %r" % type(obj).__name__)


def table_from(soa, score):
    """The junction table of layout `soa` (the engine's fragment fields) and per-fragment scores `score` (NaN: no score).  One row per
    fragment with a successor in a linear contig, ordered by (contig, position); `position` is the left fragment's, `join_bp` the offset of
    the join in its contig (end of the left fragment)."""
    nxt = np.asarray(soa["next"], dtype=np.int64)
    circ = np.asarray(soa["circ"], dtype=np.int64)
    f = np.nonzero((nxt >= 0) & (circ != 1))[0]
    contig = np.asarray(soa["id_c"], dtype=np.int64)[f]
    pos = np.asarray(soa["pos"], dtype=np.int64)[f]
    order = np.lexsort((pos, contig))
    f = f[order]
    g = nxt[f]
    ori = np.asarray(soa["ori"], dtype=np.int64)
    start = np.asarray(soa["start_bp"], dtype=np.int64)
    length = np.asarray(soa["len_bp"], dtype=np.int64)
    return {"contig": contig[order], "position": pos[order], "left_frag": f, "right_frag": g, "left_ori": ori[f], "right_ori": ori[g],
            "join_bp": start[f] + length[f], "score": np.asarray(score, dtype=np.float64)[f]}


def junction_table(sampler_or_engine):
    """The junctions of the engine's current layout in contig order: a dict of numpy columns COLUMNS."""
    e = _engine(sampler_or_engine)
    score, _ = e.junction_scores()
    return table_from(e.download_frags(), score)


def _write_tsv(path, table, columns, n_int):
    n = len(table["score"])
    with open(path, "w") as fh:
        fh.write("\t".join(columns) + "\n")
        for i in range(n):
            row = [str(int(table[c][i])) for c in columns[:n_int]]
            for c in columns[n_int:]:
                s = float(table[c][i])
                row.append("nan" if not np.isfinite(s) else repr(s))
            fh.write("\t".join(row) + "\n")
    return n


def write_junctions_tsv(path, table):
    """Write `table` (junction_table's dict) as a TSV file with a header line; scores with 17 significant digits, NaN as 'nan'."""
    return _write_tsv(path, table, COLUMNS, len(COLUMNS) - 1)


def support_table(sampler_or_engine, seed, n_rep, threshold=0.0):
    """The junctions of the engine's current layout in contig order with their bootstrap support: table_from's columns plus `support`
    (the fraction of the n_rep replicates scoring above `threshold`), `boot_mean`, `boot_min` and `boot_max` of the replicate scores
    (NaN where there is no score).  A function of (layout, contacts, seed, n_rep, threshold) alone."""
    e = _engine(sampler_or_engine)
    b = e.junction_bootstrap(seed, n_rep, threshold)
    t = table_from(e.download_frags(), b["J"])
    f = t["left_frag"]
    t.update({"support": b["support"][f], "boot_mean": b["mean"][f], "boot_min": b["min"][f], "boot_max": b["max"][f]})
    return t


def write_support_tsv(path, table):
    """Write `table` (support_table's dict) as a TSV file with a header line SUPPORT_COLUMNS; floats as write_junctions_tsv writes them."""
    return _write_tsv(path, table, SUPPORT_COLUMNS, len(COLUMNS) - 1)
