"""graal_end_links on C5-size layouts (bench.py's 50,000-fragment / 20 M-contact stand-in), next to graal_eval_full_q on the same layouts.

    python tools/links_c5.py [--reps N] [--nnz N]      one JSON line per layout: ms per call (min / median / max) incl. the fetch, links
    rocprofv3 --kernel-trace --stats -d D -o ln -- python tools/links_c5.py --reps 5     per-kernel times

Layouts: "late" (the map's 7 original contigs, min_frags 1), "late_ref_trans_accu" (the same under the sampler's default mode
GRAAL_MODE_REF_TRANS_ACCU: the quirk passes run only with bins of mixed RF counts), "contigs_of_8" (the original order cut into contigs
of 8 fragments, min_frags 1) and "exploded" (every fragment its own contig, min_frags 2: no links, the floor of the call).
With --mixed: the same map at n_sub 3 with RF counts 1..4 (the bins of a pyramid level, mixed RF counts) under GRAAL_MODE_REF_TRANS_ACCU,
late stage and contigs of 8, where the quirk passes (k_ln_mirror, k_ln_quirk) run; and the late stage with the mode off next to it.
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
    return {"min": ms[0], "median": ms[len(ms) // 2], "max": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--mixed", action="store_true", help="n_sub 3 with mixed RF counts, under and without GRAAL_MODE_REF_TRANS_ACCU")
    args = ap.parse_args()
    from graal_amd import synth
    from graal_amd.lib import Engine
    from bench import exploded_layout
    from tools.junctions_c5 import chopped
    if args.mixed:
        P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=3, seed=20141217, accu=("random", 1, 4))
    else:
        P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
        e.set_params(P["param_simu"])
        if args.mixed:
            cases = (("mixed_late", P["S_o_A_frags"], 1, False), ("mixed_late_ref_trans_accu", P["S_o_A_frags"], 1, True),
                     ("mixed_contigs_of_8_ref_trans_accu", chopped(P, 8), 1, True))
        else:
            cases = (("late", P["S_o_A_frags"], 1, False), ("late_ref_trans_accu", P["S_o_A_frags"], 1, True),
                     ("contigs_of_8", chopped(P, 8), 1, False), ("exploded", exploded_layout(P), 2, False))
        for name, s, mf, quirk in cases:
            e.set_mode(ref_trans_accu=quirk)
            e.upload_frags(s)
            e.relabel_contigs()
            ln = timed(lambda: e.end_links_q(mf), args.reps)
            full = timed(e.eval_full_q, args.reps)
            a, b, q, c, st = e.end_links_q(mf)
            print(json.dumps({"layout": name, "n_sub": 3 if args.mixed else 1, "min_frags": mf, "ref_trans_accu": quirk, "fragments": int(len(s["pos"])),
                              "contacts": int(len(P["coo_row"])), "longest_contig": int(np.max(s["l_cont"])), "links": int(len(a)),
                              "links_valid": int((st == 0).sum()), "end_links_ms": ln, "eval_full_q_ms": full,
                              "ratio_median": ln["median"] / full["median"]}), flush=True)
        e.set_mode(ref_trans_accu=False)
    finally:
        e.close()


if __name__ == "__main__":
    main()
