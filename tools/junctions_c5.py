"""graal_junction_scores on C5-size layouts (bench.py's 50,000-fragment / 20 M-contact stand-in), next to graal_eval_full_q on the same layouts.

    python tools/junctions_c5.py [--reps N] [--nnz N]      one JSON line per layout: ms per call (min / median / max), incl. the copy to the host
    rocprofv3 --kernel-trace --stats -d D -o jn -- python tools/junctions_c5.py --reps 5     per-kernel times

Layouts: "exploded" (every fragment its own contig: where bench.py's headline region starts), "contigs_of_8" (the original order cut
into contigs of 8 fragments: short contigs, as early in a run) and "late" (the map's 7 original contigs, up to ~10k fragments each).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def chopped(P, k):
    s = {key: np.array(v, dtype=np.int32, copy=True) for key, v in P["S_o_A_frags"].items()}
    n = len(s["pos"])
    pos = np.zeros(n, np.int64)
    cid = np.zeros(n, np.int64)
    c = -1
    for f in range(n):          # (fragments of a contig are consecutive ids in synth layouts)
        if s["pos"][f] == 0 or pos[f - 1] == k - 1:
            c += 1
            pos[f] = 0
        else:
            pos[f] = pos[f - 1] + 1
        cid[f] = c
    lc = np.bincount(cid)
    start = np.zeros(n, np.int64)
    for f in range(1, n):
        start[f] = 0 if pos[f] == 0 else start[f - 1] + s["len_bp"][f - 1]
    s["pos"][:] = pos; s["id_c"][:] = cid; s["start_bp"][:] = start; s["ori"][:] = 1; s["circ"][:] = 0
    s["l_cont"][:] = lc[cid]
    s["l_cont_bp"][:] = np.bincount(cid, weights=s["len_bp"]).astype(np.int64)[cid]
    idx = np.arange(n)
    s["prev"][:] = np.where(pos == 0, -1, idx - 1)
    s["next"][:] = np.where(pos == lc[cid] - 1, -1, idx + 1)
    return s


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    args = ap.parse_args()
    from graal_amd import synth
    from graal_amd.lib import Engine
    P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bench import exploded_layout
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
            full = timed(e.eval_full_q, args.reps)
            q, st = e.junction_scores_q()
            print(json.dumps({"layout": name, "fragments": int(len(st)), "contacts": int(len(P["coo_row"])),
                              "longest_contig": int(np.max(s["l_cont"])), "junctions": int((st == 0).sum()),
                              "junction_scores_ms": jn, "eval_full_q_ms": full, "ratio_median": jn["median"] / full["median"]}), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
