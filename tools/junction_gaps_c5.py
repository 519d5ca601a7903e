"""graal_junction_gaps on C5-size layouts (bench.py's 50,000-fragment / 20 M-contact stand-in): one call of G gap values next to G times
one graal_junction_scores call, measured in the same process on the same engine.

    python tools/junction_gaps_c5.py [--reps N] [--gaps G] [--nnz N] [--out FILE]     one JSON line per layout, and the table as markdown

Per layout: ms per call (min / median / max of --reps calls after one warm-up call, wall time including the copies of the per-fragment
columns to the host) of graal_junction_scores, of the gap call without the profile matrix, with it (q_gap: G * n int64 copied to the
host), and of the gap call on the first 8 and 16 values of the grid (the slope per gap value: what a value costs beyond the call's
own junction pass); `ratio` = gap call without the matrix / (G * junction scores).  The expectation, not asserted anywhere: well under
G junction calls -- one slot build, one stream of the list, G + 1 model evaluations per pair against 2 * G.

Layouts: tools/junctions_c5.py's -- "exploded" (every fragment its own contig), "contigs_of_8" and "late" (the map's 7 original contigs).
The grid: graal_amd.junctions.default_gap_grid (0, then a quarter of the median bin length up to the model's d_max).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def markdown(rows, args, grid):
    out = ["# graal_junction_gaps at C5 size (one MI355X)", "",
           "`python tools/junction_gaps_c5.py --reps %d`: bench.py's stand-in map (%d fragments, n_sub 1, %d contacts), G = %d gap values"
           % (args.reps, rows[0]["fragments"], rows[0]["contacts"], len(grid)),
           "(0, then %.3f .. %.1f kb, geometric), drop 1.92.  Wall time per call including the copies of the per-fragment columns to the host;"
           % (grid[1], grid[-1]),
           "medians of %d calls after one warm-up call, every call timed in the same process on the same engine.  \"G junction calls\" is"
           % args.reps,
           "G x the median of one `graal_junction_scores` call.", "",
           "| layout | junctions scored | one junction call (ms) | G junction calls (ms) | gap call, G = %d (ms) | ratio | 8 values (ms) | 16 values (ms) | copy of `q_gap` on top (ms) |"
           % len(grid), "|---|---:|---:|---:|---:|---:|---:|---:|---:|"]
    for r in rows:
        out.append("| %s | %d | %.3f | %.1f | %.3f (min %.3f) | %.3f | %.3f | %.3f | %.2f |"
                   % (r["layout"], r["junctions"], r["junction_scores_ms"]["median"], r["g_junction_calls_ms"], r["gaps_ms"]["median"],
                      r["gaps_ms"]["min"], r["ratio"], r["gaps_8_ms"]["median"], r["gaps_16_ms"]["median"], r["q_gap_copy_ms"]))
    out += ["", "Junctions whose interval is open towards a cut (`hi` at the last grid point): "
            + ", ".join("%s %d" % (r["layout"], r["open"]) for r in rows) + "; with the maximum at gap 0: "
            + ", ".join("%s %d" % (r["layout"], r["best_zero"]) for r in rows) + ".", "", "Raw lines:", "", "```"]
    out += [json.dumps(r) for r in rows] + ["```", ""]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--gaps", type=int, default=32)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "junction_gaps_c5.md"))
    args = ap.parse_args()
    from graal_amd import junctions, synth
    from graal_amd.lib import Engine, Q_SCALE
    from bench import exploded_layout
    from junctions_c5 import chopped, timed
    P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)
    grid = junctions.default_gap_grid(float(P["param_simu"][5]), args.gaps,
                                      median_bin_kb=float(np.median(P["S_o_A_frags"]["len_bp"])) / 1000.0)
    drop_q = int(round(1.92 * Q_SCALE))
    rows = []
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
        e.set_params(P["param_simu"])
        for name, s in (("exploded", exploded_layout(P)), ("contigs_of_8", chopped(P, 8)), ("late", P["S_o_A_frags"])):
            e.upload_frags(s)
            e.relabel_contigs()
            jn = timed(e.junction_scores_q, args.reps)
            gaps = timed(lambda: e.junction_gaps_q(grid, drop_q), args.reps)
            with_prof = timed(lambda: e.junction_gaps_q(grid, drop_q, profile=True), args.reps)
            g8 = timed(lambda: e.junction_gaps_q(grid[:8], drop_q), args.reps)
            g16 = timed(lambda: e.junction_gaps_q(grid[:16], drop_q), args.reps)
            b = e.junction_gaps_q(grid, drop_q)
            ok = b["status"] == 0
            rows.append({"layout": name, "fragments": int(len(ok)), "contacts": int(len(P["coo_row"])), "gaps": len(grid),
                         "longest_contig": int(np.max(s["l_cont"])), "junctions": int(ok.sum()),
                         "open": int((b["hi"][ok] == len(grid) - 1).sum()), "best_zero": int((b["best"][ok] == 0).sum()),
                         "junction_scores_ms": jn, "gaps_ms": gaps, "gaps_with_q_gap_ms": with_prof, "gaps_8_ms": g8, "gaps_16_ms": g16,
                         "q_gap_copy_ms": with_prof["median"] - gaps["median"], "g_junction_calls_ms": len(grid) * jn["median"],
                         "ratio": gaps["median"] / (len(grid) * jn["median"])})
            print(json.dumps(rows[-1]), flush=True)
    finally:
        e.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(markdown(rows, args, grid))


if __name__ == "__main__":
    main()
