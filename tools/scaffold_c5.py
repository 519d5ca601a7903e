"""Scaffolding on C5-size layouts (bench.py's 50,000-fragment / 20 M-contact stand-in).

    python tools/scaffold_c5.py [--reps N] [--nnz N]      one JSON line per measurement -> profiles/scaffold_c5.md

  - "best_vs_table": contigs of 8 fragments, min_frags 1: graal_end_links_best (incl. the copy of the per-end arrays and the mutual
    list) next to graal_end_links + its fetch (the whole sorted table), ms per call;
  - "edit_round": the same layout, one round's joins (its mutual-best links, cycles broken) applied by graal_edit_layout, ms per call
    (the layout is uploaded again between calls, outside the timing);
  - "scaffold_80": the map cut into pieces of 80 fragments (original order and orientation), graal_amd.scaffold.scaffold to the end:
    wall time, rounds, joins and contigs;
  - "exploded_min_frags_1": every fragment its own contig, graal_end_links_best at min_frags 1: ms, or the refusal's message when the
    candidate table is over the GRAAL_LINKS_MAX_BYTES budget.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps, before=None):
    if before:
        before()
    fn()
    ms = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    args = ap.parse_args()
    from graal_amd import scaffold, synth
    from graal_amd.lib import Engine, GraalError
    from bench import exploded_layout
    from tools.junctions_c5 import chopped
    P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
        e.set_params(P["param_simu"])
        s8 = chopped(P, 8)
        e.upload_frags(s8)
        e.relabel_contigs()
        best = timed(lambda: e.end_links_best(1), args.reps)
        table = timed(lambda: e.end_links_q(1), max(2, args.reps // 2))
        _, _, mutual = e.end_links_best(1)
        idc = e.download_frags()["id_c"]
        a, b, _ = scaffold.plan_joins(mutual, 0.0, lambda end: idc[end >> 1])
        print(json.dumps({"measure": "best_vs_table", "fragments": int(len(s8["pos"])), "contacts": int(len(P["coo_row"])),
                          "mutual": int(len(mutual[0])), "end_links_best_ms": best, "end_links_and_fetch_ms": table,
                          "ratio_median": table["median"] / best["median"]}), flush=True)
        joins = np.stack([a, b], axis=1)
        ed = timed(lambda: e.edit_layout([], joins), args.reps, before=lambda: e.upload_frags(s8))
        print(json.dumps({"measure": "edit_round", "joins": int(len(a)), "edit_layout_ms": ed}), flush=True)
        s80 = chopped(P, 80)
        e.upload_frags(s80)
        t0 = time.perf_counter()
        rec = scaffold.scaffold(e, rounds=50)
        dt = time.perf_counter() - t0
        print(json.dumps({"measure": "scaffold_80", "pieces": int(len(np.unique(s80["id_c"]))), "seconds": dt,
                          "rounds": len(rec) - 1, "record": rec}), flush=True)
        e.upload_frags(exploded_layout(P))
        e.relabel_contigs()
        try:
            ms = timed(lambda: e.end_links_best(1), 2)
            print(json.dumps({"measure": "exploded_min_frags_1", "end_links_best_ms": ms}), flush=True)
        except GraalError as err:
            print(json.dumps({"measure": "exploded_min_frags_1", "refused": str(err)}), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
