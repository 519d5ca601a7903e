"""Rings: score closing each contig into a ring, or opening each ring at its wrap (Engine.ring_scores), and close those the data prefer.

    ring_table(engine, soa)                                       -- one row per contig, as a dict of columns (see COLUMNS)
    plan_rings(table, min_score=0.0, open_rings=False)            -- the rows to apply
    close_rings(sampler_or_engine, min_score=0.0, open_rings=False) -- score, plan, apply, evaluate; returns the record
    write_rings_tsv(path, table) / write_close_rings_tsv(path, record)

R = logL(the layout with the contig in the other topology, every coordinate kept) - logL(layout), in the engine's exact arithmetic.
Contigs share no sub-fragment pair, so the scores of different contigs add exactly: everything is applied at once and there are no
rounds.  The ring price is the reference's: only the pairs less than d_max apart ALONG the contig are priced differently in a ring, so
a contig shorter than d_max gets a true ring model and a longer one is judged by its in-window pairs alone; contacts between head and
tail further apart carry nothing.
"""
import numpy as np

from . import scaffold as _sc
from .lib import Q_SCALE, RING_CLOSE, RING_OPEN

COLUMNS = ("contig", "head", "frags", "bp", "circ", "score", "contacts", "status")
RECORD_COLUMNS = ("closed", "opened", "contigs", "logL_before", "logL", "expected_gain", "kept")


def ring_table(engine, soa=None):
    """One row per contig of the engine's current layout (soa: its downloaded fields), in label order: the contig's label, its
    position-0 fragment, its fragments and bp, circ, the score (NaN for RING_SINGLE / RING_NONFINITE), the wrap-side contacts and the
    status byte."""
    soa = engine.download_frags() if soa is None else soa
    score, contacts, st = engine.ring_scores()
    head = np.nonzero(np.asarray(soa["pos"]) == 0)[0]
    head = head[np.argsort(np.asarray(soa["id_c"])[head], kind="stable")]
    return {"contig": np.asarray(soa["id_c"], dtype=np.int64)[head], "head": head.astype(np.int64),
            "frags": np.asarray(soa["l_cont"], dtype=np.int64)[head], "bp": np.asarray(soa["l_cont_bp"], dtype=np.int64)[head],
            "circ": np.asarray(soa["circ"], dtype=np.int64)[head], "score": score[head], "contacts": contacts[head], "status": st[head]}


def plan_rings(table, min_score=0.0, open_rings=False):
    """The row indices to apply: RING_CLOSE rows with score > min_score; with open_rings also the RING_OPEN rows with score > min_score."""
    st = np.asarray(table["status"])
    with np.errstate(invalid="ignore"):
        good = np.asarray(table["score"], dtype=np.float64) > float(min_score)
    take = (st == RING_CLOSE) | ((st == RING_OPEN) if open_rings else False)
    return np.nonzero(good & take)[0]


def _window_terms(soa, heads, reach_bp):
    """Fragment pairs inside the window (and one own-bin pair per fragment) of the contigs with these position-0 fragments."""
    idc, pos = np.asarray(soa["id_c"]), np.asarray(soa["pos"])
    start, ln = np.asarray(soa["start_bp"], dtype=np.int64), np.asarray(soa["len_bp"], dtype=np.int64)
    total = 0
    for h in heads:
        m = np.nonzero(idc == idc[h])[0]
        m = m[np.argsort(pos[m])]
        jmax = np.searchsorted(start[m], start[m] + ln[m] + reach_bp, side="right") - 1
        total += int(np.maximum(jmax - np.arange(len(m)), 0).sum()) + len(m)
    return total


def close_rings(sampler_or_engine, min_score=0.0, open_rings=False):
    """Score every contig, close the linear ones scoring above min_score (open_rings: and open the rings scoring above it, each by a
    cut at its wrap) in one call each, relabel and evaluate in full.  The applied scores add exactly, so logL must rise by their sum to
    the roundings: one unit of 2^-30 per term (contact or fragment pair inside the window), plus 1e-9 of |logL| before and after for
    the float64 sums of the terms themselves.  If it does not, the layout from before is uploaded again and the record says so
    (kept 0).  Returns the record: a dict with the keys RECORD_COLUMNS and the table and the rows applied."""
    obj = sampler_or_engine
    e = _sc._engine(obj)
    logl, nc = _sc._evaluate(e)
    before = e.download_frags()                  # (relabelled: the layout a restore uploads)
    table = ring_table(e, before)
    rows = plan_rings(table, min_score, open_rings)
    st = np.asarray(table["status"])[rows]
    close, opened = rows[st == RING_CLOSE], rows[st == RING_OPEN]
    rec = {"closed": int(len(close)), "opened": int(len(opened)), "contigs": nc, "logL_before": logl, "logL": logl,
           "expected_gain": float(np.asarray(table["score"])[rows].sum()) if len(rows) else 0.0, "kept": 1, "table": table, "rows": rows}
    if len(rows) == 0:
        return rec
    if len(close):
        if hasattr(obj, "close_rings") and obj is not e:
            obj.close_rings(table["head"][close])
        else:
            e.close_rings(table["head"][close])
    if len(opened):
        idc, pos, lc = (np.asarray(before[k]) for k in ("id_c", "pos", "l_cont"))
        last = {int(idc[f]): int(f) for f in np.nonzero(pos == lc - 1)[0]}
        _sc._edit(obj, e, [last[int(c)] for c in table["contig"][opened]], np.zeros((0, 2), dtype=np.int64))
    new_logl, nc = _sc._evaluate(e)
    par = getattr(e, "param", None)
    reach = int(np.ceil(np.float64(np.float32(par[5])) * 1000.0)) + 1000 if par is not None else int(np.max(before["l_cont_bp"]))
    terms = _window_terms(before, table["head"][rows], reach) + int(getattr(e, "nnz", 0)) + 1
    tol = 1e-9 * (abs(logl) + abs(new_logl)) + terms / Q_SCALE
    rec.update({"contigs": nc, "logL": new_logl, "tolerance": tol})
    if not abs((new_logl - logl) - rec["expected_gain"]) <= tol:      # (NaN included)
        rec["kept"] = 0
        _sc._restore(obj, e, before)
        _sc._evaluate(e)
    return rec


def write_rings_tsv(path, table):
    """ring_table's columns as a TSV file with a header line; scores with 17 significant digits (nan where there is none)."""
    n = len(table["contig"])
    with open(path, "w") as fh:
        fh.write("\t".join(COLUMNS) + "\n")
        for i in range(n):
            fh.write("\t".join(repr(float(table[c][i])) if c == "score" else str(int(table[c][i])) for c in COLUMNS) + "\n")
    return n


def write_close_rings_tsv(path, record):
    """close_rings' record as a TSV file: a header line and one row; the likelihoods with 17 significant digits."""
    with open(path, "w") as fh:
        fh.write("\t".join(RECORD_COLUMNS) + "\n")
        fh.write("\t".join(repr(float(record[c])) if c in ("logL_before", "logL", "expected_gain") else str(int(record[c]))
                           for c in RECORD_COLUMNS) + "\n")
    return 1
