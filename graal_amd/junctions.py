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

Junction gaps (graal_junction_gaps): the layout model lets contigs abut; the contact model prices a pair by its distance, so the gap
behind a fragment is a parameter the data can estimate.  The likelihood profile of that gap over a grid of values, every junction in
one GPU call: the grid value with the largest profile, and the interval within `drop` log-likelihood units of it (1.92: the 95 %
likelihood-ratio interval of one parameter).

    default_gap_grid(d_max_kb, points=32, min_kb=None)             -- 0, then geometric values from min_kb up to and including d_max
    gap_table(sampler_or_engine, gap_kb=None, drop=1.92)           -- junction_table's columns plus GAP_COLUMNS[len(COLUMNS):]
    write_gaps_tsv(path, table)                                    -- the same as a TSV file
"""
import numpy as np

from .lib import Engine, JUNCTION_CIRCULAR, JUNCTION_END, JUNCTION_NONFINITE, JUNCTION_VALID

COLUMNS = ("contig", "position", "left_frag", "right_frag", "left_ori", "right_ori", "join_bp", "score")
SUPPORT_COLUMNS = COLUMNS + ("support", "boot_mean", "boot_min", "boot_max")
GAP_COLUMNS = COLUMNS + ("gap_kb", "gap_score", "gap_lo_kb", "gap_hi_kb", "gap_open")
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


def default_gap_grid(d_max_kb, points=32, min_kb=None, median_bin_kb=None):
    """The gap grid of `points` float32 values (2 .. 64): 0, then points - 1 geometric values from min_kb up to and including d_max_kb (a
    gap as wide as the window is a cut: the last row of the profile is minus the junction score).  min_kb defaults to a quarter of
    median_bin_kb, the median bin length."""
    points = int(points)
    if not 2 <= points <= 64:
        raise ValueError("a gap grid has 2 .. 64 points, not %d" % points)
    d_max = float(np.float32(d_max_kb))
    if min_kb is None:
        if median_bin_kb is None:
            raise ValueError("default_gap_grid needs min_kb or median_bin_kb")
        min_kb = 0.25 * float(median_bin_kb)
    min_kb = float(min_kb)
    if not (0.0 < min_kb < d_max or (points == 2 and 0.0 < min_kb <= d_max)):
        raise ValueError("the smallest gap %r kb must lie in (0, d_max = %r kb)" % (min_kb, d_max))
    g = np.concatenate([[0.0], np.geomspace(min_kb, d_max, points - 1) if points > 2 else [d_max]]).astype(np.float32)
    g[-1] = np.float32(d_max_kb)
    if not (np.diff(g) > 0).all():
        raise ValueError("the grid does not ascend in float32: fewer points, or a larger smallest gap")
    return g


def gap_table_from(soa, gaps, gap_kb):
    """gap_table's dict from the layout `soa`, Engine.junction_gaps' dict `gaps` and the grid: table_from's columns, then per junction
    gap_kb (the grid value with the largest profile), gap_score (that profile value: logL with the gap - logL without), gap_lo_kb /
    gap_hi_kb (the interval within the drop) and gap_open (1 when the interval reaches the last grid point: the data do not bound the
    gap from above, the join is no better than a cut)."""
    t = table_from(soa, gaps["J"])
    f = t["left_frag"]
    last = len(np.asarray(gap_kb).reshape(-1)) - 1
    ok = np.isfinite(np.asarray(gaps["gap_score"], dtype=np.float64)[f])
    t.update({"gap_kb": gaps["gap_kb"][f], "gap_score": gaps["gap_score"][f], "gap_lo_kb": gaps["gap_lo_kb"][f],
              "gap_hi_kb": gaps["gap_hi_kb"][f],
              "gap_open": np.where(ok, (np.asarray(gaps["hi"])[f] == last).astype(np.float64), np.nan)})
    return t


def gap_table(sampler_or_engine, gap_kb=None, drop=1.92, points=32, max_kb=None):
    """The junctions of the engine's current layout in contig order with their gap estimates (GAP_COLUMNS).  gap_kb: the grid (kb);
    default default_gap_grid(max_kb or the model's d_max, points) with a quarter of the median bin length as the smallest gap."""
    e = _engine(sampler_or_engine)
    soa = e.download_frags()
    if gap_kb is None:
        d_max = float(e.param[5]) if max_kb is None else float(max_kb)
        gap_kb = default_gap_grid(d_max, points, median_bin_kb=float(np.median(np.asarray(soa["len_bp"], dtype=np.float64))) / 1000.0)
    gap_kb = np.ascontiguousarray(gap_kb, dtype=np.float32).reshape(-1)
    return gap_table_from(soa, e.junction_gaps(gap_kb, drop), gap_kb)


def write_gaps_tsv(path, table):
    """Write `table` (gap_table's dict) as a TSV file with a header line GAP_COLUMNS; floats as write_junctions_tsv writes them."""
    return _write_tsv(path, table, GAP_COLUMNS, len(COLUMNS) - 1)
