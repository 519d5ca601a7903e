"""graal_junction_bootstrap on C5-size layouts (bench.py's 50,000-fragment / 20 M-contact stand-in): one call of R replicates next to R
times one graal_junction_scores call, measured in the same process on the same engine.

    python tools/junction_boot_c5.py [--reps N] [--replicates R] [--nnz N]      one JSON line per layout

Per layout: ms per call (min / median / max of --reps calls after one warm-up call, wall time including the copies of the per-fragment
columns to the host) of graal_junction_scores, of the bootstrap without the replicate matrix, and of the bootstrap with it (q_rep: R * n
int64 copied to the host batch by batch); `q_rep_copy_ms` is the difference of the last two medians; `ratio` = bootstrap without the
matrix / (R * junction scores).  R junction calls are the floor of the naive route, which also resamples on the host and uploads the
contact list R times: neither is in the figure.

Layouts: tools/junctions_c5.py's -- "exploded" (every fragment its own contig), "contigs_of_8" and "late" (the map's 7 original contigs).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    from graal_amd import synth
    from graal_amd.lib import Engine
    from bench import exploded_layout
    from junctions_c5 import chopped, timed
    R = args.replicates
    P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)
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
            boot = timed(lambda: e.junction_bootstrap_q(args.seed, R), args.reps)
            with_rep = timed(lambda: e.junction_bootstrap_q(args.seed, R, 0, replicates=True), args.reps)
            b = e.junction_bootstrap_q(args.seed, R)
            ok = b["status"] == 0
            print(json.dumps({"layout": name, "fragments": int(len(ok)), "contacts": int(len(P["coo_row"])), "replicates": R,
                              "longest_contig": int(np.max(s["l_cont"])), "junctions": int(ok.sum()),
                              "mean_support": float(b["support"][ok].mean() / R) if ok.any() else None,
                              "junction_scores_ms": jn, "bootstrap_ms": boot, "bootstrap_with_q_rep_ms": with_rep,
                              "q_rep_copy_ms": with_rep["median"] - boot["median"], "r_junction_calls_ms": R * jn["median"],
                              "ratio": boot["median"] / (R * jn["median"])}), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
