"""graal_block_swaps on C5-size layouts (bench.py's 50,000-fragment / 20 M-contact stand-in), next to graal_block_flips and
graal_block_excisions for the same spans as blocks, graal_ring_scores and graal_eval_full_q, on the same engine.

    python tools/swaps_c5.py [--reps N] [--nnz N]      one JSON line per (layout, tiling set): ms per call (min / median / max)
    rocprofv3 --kernel-trace --stats -d D -o sw -- python tools/swaps_c5.py --reps 3     per-kernel times

Layouts: "late" (the map's 7 original contigs) and "contigs_of_8" (the original order cut into contigs of 8 fragments).  A tiling set
(span m, split a) is graal_amd.swaps.tilings' set at offset 0: the swaps of a run of a fragments with the m - a behind it that start
0, m, 2 m, ... fragments into every contig -- one call of a round of swap_rounds.  The flips and the excisions calls get the same
spans as blocks.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return {"min": round(ms[0], 3), "median": round(ms[len(ms) // 2], 3), "max": round(ms[-1], 3)}


def one_set(soa, span, split):
    """The tiling set (span, split) at offset 0."""
    from graal_amd import swaps
    pos = np.asarray(soa["pos"])
    for first, mid, last in swaps.tilings(soa, None, span):
        if pos[last[0]] - pos[first[0]] + 1 == span and pos[mid[0]] - pos[first[0]] + 1 == split:
            return first, mid, last
    raise ValueError("no such set")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    args = ap.parse_args()
    from graal_amd import synth
    from graal_amd.lib import Engine
    from tools.junctions_c5 import chopped
    P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
        e.set_params(P["param_simu"])
        for name, s, sets in (("late", P["S_o_A_frags"], ((2, 1), (4, 2), (8, 4))), ("contigs_of_8", chopped(P, 8), ((2, 1), (4, 2)))):
            e.upload_frags(s)
            e.relabel_contigs()
            s = e.download_frags()
            full = timed(e.eval_full_q, args.reps)
            rings = timed(e.ring_scores_q, args.reps)
            for span, split in sets:
                first, mid, last = one_set(s, span, split)
                sw = timed(lambda: e.block_swaps_q(first, mid, last), args.reps)
                fl = timed(lambda: e.block_flips_q(first, last), args.reps)
                ex = timed(lambda: e.block_excisions_q(first, last), args.reps)
                q, c, st = e.block_swaps_q(first, mid, last)
                print(json.dumps({"layout": name, "span": span, "split": split, "fragments": int(len(s["pos"])), "contacts": int(len(P["coo_row"])),
                                  "longest_contig": int(np.max(s["l_cont"])), "swaps": int(len(first)), "swaps_valid": int((st == 0).sum()),
                                  "block_swaps_ms": sw, "block_flips_ms": fl, "block_excisions_ms": ex, "ring_scores_ms": rings,
                                  "eval_full_q_ms": full,
                                  "swaps_over_flips": round(sw["median"] / fl["median"], 2),
                                  "swaps_over_full": round(sw["median"] / full["median"], 2)}), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
