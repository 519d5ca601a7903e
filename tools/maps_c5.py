"""graal_layout_maps on C5-size layouts (bench.py's 50,000-fragment / 20 M-contact stand-in), next to graal_eval_full_q on the same layouts
and image.matrix_image of the same list on one host core.

    python tools/maps_c5.py [--reps N] [--nnz N] [--max-px N] [--no-host]      one JSON line per layout: ms (min / median / max) of the call
                                                                               without the fetch, of the fetch, and of the two yardsticks
    rocprofv3 --kernel-trace --stats -d D -o maps -- python tools/maps_c5.py --reps 5 --no-host     per-kernel times

Layouts: "exploded" (every fragment its own contig: where bench.py's headline region starts) and "late" (the map's 7 original contigs, up
to ~10k fragments each).
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--nnz", type=int, default=20_000_000)
    ap.add_argument("--max-px", type=int, default=2048)
    ap.add_argument("--no-host", action="store_true", help="skip image.matrix_image (tens of seconds on one core)")
    args = ap.parse_args()
    from graal_amd import image, synth
    from graal_amd.lib import Engine
    from bench import exploded_layout
    P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)
    coo = (P["coo_row"], P["coo_col"], P["coo_val"])
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.upload_contacts(*coo)
        e.set_params(P["param_simu"])
        for name, s in (("exploded", exploded_layout(P)), ("late", P["S_o_A_frags"])):
            e.upload_frags(s)
            e.relabel_contigs()
            call = timed(lambda: e.layout_maps_compute(args.max_px), args.reps)
            m, b = e.layout_maps_compute(args.max_px)
            bufs = [np.zeros((m, m), dtype=np.float32) for _ in range(3)]
            fetch = timed(lambda: e.layout_maps_fetch(*bufs), args.reps)
            full = timed(e.eval_full_q, args.reps)
            out = {"layout": name, "fragments": int(len(s["pos"])), "contacts": int(len(coo[0])), "longest_contig": int(np.max(s["l_cont"])),
                   "max_px": args.max_px, "m": m, "bin": b, "layout_maps_ms": call, "fetch_ms": fetch, "eval_full_q_ms": full,
                   "ratio_median": call["median"] / full["median"]}
            if not args.no_host:
                O, E, R, pix, b, bad = e.layout_maps(args.max_px)
                order = np.argsort(pix, kind="stable")       # (one sub-fragment per bin: a stable sort of the pixels is an order with these pixels)
                t0 = time.perf_counter()
                want = image.matrix_image(coo, order, args.max_px)
                out["matrix_image_host_ms"] = 1e3 * (time.perf_counter() - t0)
                out["observed_equals_host"] = bool(np.array_equal(O, want))
                out["bad_pixels"] = int(bad)
            print(json.dumps(out), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
