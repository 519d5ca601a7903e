"""End links: how strongly the data support joining two contig ends (graal_end_links, HIP on the GPU) -- the scaffold graph of a layout.

An end is one side of a linear contig: end = 2 * fragment + side, side 0 the contig's head, side 1 its tail.  For two ends of different
contigs, score = logL(the layout with the two contigs joined at those ends) - logL(layout) in the engine's exact arithmetic: the first
contig oriented so that its end is its tail, the second after it so that its end is its head.  A positive score means the data prefer the
join.  Only pairs of ends with at least one contact inside the contact model's window (d_max) in the joined orientation are listed: any
other pair would score only its negative expected mass.

    link_table(sampler_or_engine, min_frags=1)   -- the listed links as a dict of columns (see COLUMNS), sorted by (end_a, end_b)
    best_links(table, k)                         -- the k best partners of every end (a dict of columns, see BEST_COLUMNS)
    mutual_best(table)                           -- the links whose two ends are each other's best partner with a positive score
    write_links_tsv(path, table)                 -- one tab-separated row per link, with a header line

Link support (graal_end_links_bootstrap): a Poisson bootstrap of the read pairs -- every contact's count redrawn as Poisson(count), n_rep
times, in one GPU call.  Per listed link: support, the fraction of the resampled datasets in which the join still scores above 0, and
mutual, the fraction in which it also is the join both of its ends choose (each the other's best partner) -- the number a phylogeny
program prints beside a branch.  Under one seed replicate r is the same resampled dataset as graal_amd.junctions' support replicate r.

    support_table(sampler_or_engine, seed, n_rep, min_frags=1, threshold=0.0)   -- COLUMNS plus SUPPORT_COLUMNS' last five
    write_support_tsv(path, table)                                              -- one row per link, with a header line
"""
import numpy as np

from .lib import Engine, LINK_NONFINITE, LINK_VALID

COLUMNS = ("contig_a", "frag_a", "side_a", "contig_b", "frag_b", "side_b", "contacts", "score")
BEST_COLUMNS = ("contig", "frag", "side", "rank", "partner_contig", "partner_frag", "partner_side", "contacts", "score")
SUPPORT_COLUMNS = COLUMNS + ("support", "mutual", "boot_mean", "boot_min", "boot_max")
STATUS_NAMES = {LINK_VALID: "valid", LINK_NONFINITE: "nonfinite"}


def _engine(obj):
    if isinstance(obj, Engine):
        return obj
    e = getattr(obj, "engine", None)
    if isinstance(e, Engine):
        return e
    raise TypeError("link_table takes a graal_amd Engine or a sampler that holds one (.engine), not %r" % type(obj).__name__)


def table_from(soa, end_a, end_b, contacts, score):
    """The link table of layout `soa` (the engine's fragment fields) from graal_end_links' columns (score NaN: no score)."""
    a = np.asarray(end_a, dtype=np.int64)
    b = np.asarray(end_b, dtype=np.int64)
    idc = np.asarray(soa["id_c"], dtype=np.int64)
    return {"contig_a": idc[a >> 1], "frag_a": a >> 1, "side_a": a & 1, "contig_b": idc[b >> 1], "frag_b": b >> 1, "side_b": b & 1,
            "contacts": np.asarray(contacts, dtype=np.int64), "score": np.asarray(score, dtype=np.float64)}


def link_table(sampler_or_engine, min_frags=1):
    """The links of the engine's current layout between contigs of >= min_frags fragments: a dict of numpy columns COLUMNS."""
    e = _engine(sampler_or_engine)
    a, b, score, c, _ = e.end_links(min_frags)
    return table_from(e.download_frags(), a, b, c, score)


def _directed(table):
    """Every link seen from both of its ends: (end, partner end, row) arrays."""
    ea = 2 * np.asarray(table["frag_a"], dtype=np.int64) + np.asarray(table["side_a"], dtype=np.int64)
    eb = 2 * np.asarray(table["frag_b"], dtype=np.int64) + np.asarray(table["side_b"], dtype=np.int64)
    row = np.arange(len(ea))
    return np.concatenate([ea, eb]), np.concatenate([eb, ea]), np.concatenate([row, row])


def best_links(table, k):
    """The k best partners of every end that has a scored link, best first (ties: the lower partner end first).  A dict of columns
    BEST_COLUMNS sorted by (frag, side, rank), rank 0 the best."""
    end, other, row = _directed(table)
    score = np.asarray(table["score"], dtype=np.float64)[row]
    ok = np.isfinite(score)
    end, other, row, score = end[ok], other[ok], row[ok], score[ok]
    order = np.lexsort((other, -score, end))
    end, other, row = end[order], other[order], row[order]
    first = np.concatenate([[True], end[1:] != end[:-1]]) if len(end) else np.zeros(0, bool)
    start = np.maximum.accumulate(np.where(first, np.arange(len(end)), 0))
    rank = np.arange(len(end)) - start
    keep = rank < int(k)
    end, other, row, rank = end[keep], other[keep], row[keep], rank[keep]
    own_a = (2 * np.asarray(table["frag_a"], dtype=np.int64)[row] + np.asarray(table["side_a"], dtype=np.int64)[row]) == end
    pick = lambda x, y: np.where(own_a, np.asarray(table[x], dtype=np.int64)[row], np.asarray(table[y], dtype=np.int64)[row])
    return {"contig": pick("contig_a", "contig_b"), "frag": end >> 1, "side": end & 1, "rank": rank,
            "partner_contig": pick("contig_b", "contig_a"), "partner_frag": other >> 1, "partner_side": other & 1,
            "contacts": np.asarray(table["contacts"], dtype=np.int64)[row], "score": np.asarray(table["score"], dtype=np.float64)[row]}


def mutual_best(table):
    """The rows of `table` whose two ends are each other's best partner (best_links' order) with a positive score: the joins the data
    propose.  A table with the columns COLUMNS, in the order of `table`."""
    b = best_links(table, 1)
    best = dict(zip((2 * b["frag"] + b["side"]).tolist(), (2 * b["partner_frag"] + b["partner_side"]).tolist()))
    ea = 2 * np.asarray(table["frag_a"], dtype=np.int64) + np.asarray(table["side_a"], dtype=np.int64)
    eb = 2 * np.asarray(table["frag_b"], dtype=np.int64) + np.asarray(table["side_b"], dtype=np.int64)
    score = np.asarray(table["score"], dtype=np.float64)
    keep = np.array([best.get(int(x)) == int(y) and best.get(int(y)) == int(x) for x, y in zip(ea, eb)], dtype=bool)
    keep &= np.isfinite(score) & (score > 0)
    return {c: np.asarray(table[c])[keep] for c in COLUMNS}


def write_links_tsv(path, table):
    """Write `table` (link_table's dict) as a TSV file with a header line; scores with 17 significant digits, NaN as 'nan'."""
    n = len(table["score"])
    with open(path, "w") as fh:
        fh.write("\t".join(COLUMNS) + "\n")
        for i in range(n):
            row = [str(int(table[c][i])) for c in COLUMNS[:-1]]
            s = float(table["score"][i])
            row.append("nan" if not np.isfinite(s) else repr(s))
            fh.write("\t".join(row) + "\n")
    return n


def support_table(sampler_or_engine, seed, n_rep, min_frags=1, threshold=0.0):
    """link_table's rows of the engine's current layout plus the bootstrap columns: a dict of numpy columns SUPPORT_COLUMNS (support and
    mutual are fractions of the n_rep replicates; NaN where the link has no score)."""
    e = _engine(sampler_or_engine)
    b = e.end_links_bootstrap(seed, n_rep, min_frags, threshold)
    t = table_from(e.download_frags(), b["end_a"], b["end_b"], b["contacts"], b["score"])
    t.update({"support": b["support"], "mutual": b["mutual"], "boot_mean": b["mean"], "boot_min": b["min"], "boot_max": b["max"]})
    return t


def write_support_tsv(path, table):
    """Write `table` (support_table's dict) as a TSV file with a header line; floats with 17 significant digits, NaN as 'nan'."""
    n = len(table["score"])
    ints = COLUMNS[:-1]
    with open(path, "w") as fh:
        fh.write("\t".join(SUPPORT_COLUMNS) + "\n")
        for i in range(n):
            row = [str(int(table[c][i])) for c in ints]
            for c in SUPPORT_COLUMNS[len(ints):]:
                v = float(table[c][i])
                row.append("nan" if not np.isfinite(v) else repr(v))
            fh.write("\t".join(row) + "\n")
    return n
