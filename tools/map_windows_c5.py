"""graal_map_windows on C5-size layouts (bench.py's 50,000-fragment / 20 M-contact stand-in), next to graal_layout_maps at 2048 pixels a
side -- as many pixels as 64 windows of 256 x 256 -- on the same layouts.

    python tools/map_windows_c5.py [--reps N] [--nnz N] [--full-only]     one JSON line per layout and shape: ms (min / median / max) of
                                                                          the call without the fetch, warm
    rocprofv3 --kernel-trace --stats -d D -o windows -- python tools/map_windows_c5.py --reps 5     per-kernel times

The calls return behind their own stream synchronisation, so the host clock around a call is the time until its result is on the device
and its flag word read back.  Windows lie on the diagonal, evenly spaced over the genome (what junction thumbnails are).  --full-only
times graal_layout_maps alone: with GRAAL_HIP_LIB pointing at another build of the library, that build's figure.

Layouts: "exploded" (every fragment its own contig: where bench.py's headline region starts) and "late" (the map's 7 original contigs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (windows, pixels a side, bin); 256 windows of 256 x 256 are the call's pixel budget (4096 x 4096)
SHAPES = ((1, 256, 1), (64, 256, 1), (256, 256, 1), (1024, 128, 1), (64, 256, 16))


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
    ap.add_argument("--full-only", action="store_true")
    args = ap.parse_args()
    from graal_amd import synth
    from graal_amd.lib import Engine
    from bench import exploded_layout
    P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)
    S = int(P["init_n_sub_frags"])
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
        e.set_params(P["param_simu"])
        for name, s in (("exploded", exploded_layout(P)), ("late", P["S_o_A_frags"])):
            e.upload_frags(s)
            e.relabel_contigs()
            base = {"layout": name, "fragments": int(len(s["pos"])), "contacts": int(len(P["coo_row"])), "longest_contig": int(np.max(s["l_cont"]))}
            full = timed(lambda: e.layout_maps_compute(2048), args.reps)
            print(json.dumps(dict(base, call="layout_maps", max_px=2048, ms=full)), flush=True)
            if args.full_only:
                continue
            for n_win, px, b in SHAPES:
                u0 = np.linspace(0, S - px * b, n_win).astype(np.int32) if n_win > 1 else np.array([S // 2], dtype=np.int32)
                origins = np.stack([u0, u0], axis=1)
                ms = timed(lambda: e.map_windows_compute(origins, px, px, b), args.reps)
                obs = np.zeros((n_win, px, px), dtype=np.float32)
                e.map_windows_fetch(obs, None, None, rank_of_sub=False)
                print(json.dumps(dict(base, call="map_windows", windows=n_win, px=px, bin=b, ms=ms, bad_pixels=e._windows_bad,
                                      observed_sum=float(obs.sum(dtype=np.float64)), ratio_to_full=ms["median"] / full["median"])), flush=True)
    finally:
        e.close()


if __name__ == "__main__":
    main()
