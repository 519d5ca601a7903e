"""graal_end_links_bootstrap on C5-size layouts (bench.py's 50,000-fragment / 20 M-contact stand-in): one call of R replicates next to R
times one graal_end_links call, measured in the same process.

    python tools/links_boot_c5.py [--reps N] [--replicates R] [--nnz N] [--links-lib PATH]      one JSON line per layout

Per layout: ms per call (min / median / max of --reps calls after one warm-up call, wall time, WITHOUT the fetch of the columns) of
graal_end_links and of the bootstrap without the replicate matrix; `ratio` = bootstrap / (R * end links).  R link calls are the floor
of the naive route, which also resamples on the host and uploads the contact list R times: neither is in the figure.  --links-lib: a
libgraal_hip.so of another build (the parent commit's) to time graal_end_links with, on an engine of its own in the same process.  A
refusal (the byte budget GRAAL_LINKS_MAX_BYTES) is reported with its message instead of a time.

Layouts: tools/junctions_c5.py's "late" (the map's 7 original contigs, min_frags 1), "contigs_of_8" (min_frags 1) and "exploded" (every
fragment its own contig) at min_frags 2, where no contig is eligible.
"""
import argparse
import ctypes
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
    ap.add_argument("--links-lib", default=None)
    args = ap.parse_args()
    from graal_amd import synth
    from graal_amd.lib import Engine, GraalError
    from bench import exploded_layout
    from junctions_c5 import chopped, timed
    R = args.replicates
    P = synth.make_problem(n_bins=50000, nnz=args.nnz, n_sub=1, seed=20141217)

    def links_call(eng, mf):
        m = ctypes.c_int64(0)
        eng._ck(eng._L.graal_end_links(eng._h, mf, ctypes.byref(m)), "graal_end_links")
        return int(m.value)

    def boot_call(eng, mf):
        m = ctypes.c_int64(0)
        eng._ck(eng._L.graal_end_links_bootstrap(eng._h, mf, ctypes.c_uint64(args.seed), R, 0, 0, ctypes.byref(m)), "graal_end_links_bootstrap")
        return int(m.value)

    def attempt(fn):
        try:
            fn()                                                     # (sizes the buffers: a refusal shows here)
            return timed(fn, args.reps)
        except GraalError as err:
            return {"refused": str(err)}

    def engine(lib_path=None):
        e = Engine(0)                                                # (its constructor sets every attribute the methods use)
        if lib_path:
            # the same object on a handle of the other build: only the entry points named here are called through it
            from graal_amd import lib as glib
            L = ctypes.CDLL(lib_path)
            for name in ("graal_create", "graal_destroy", "graal_last_error", "graal_set_params", "graal_upload_subfrags",
                         "graal_upload_contacts", "graal_upload_contacts_f32", "graal_upload_frags", "graal_relabel_contigs", "graal_end_links"):
                getattr(L, name).argtypes = getattr(glib.load(), name).argtypes
                getattr(L, name).restype = getattr(glib.load(), name).restype
            e._L.graal_destroy(e._h)
            e._h = ctypes.c_void_p()
            if L.graal_create(0, ctypes.byref(e._h)) != 0:
                raise SystemExit("graal_create failed in %s" % lib_path)
            e._L = L
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.upload_contacts(P["coo_row"], P["coo_col"], P["coo_val"])
        e.set_params(P["param_simu"])
        return e

    e = engine()
    ref = engine(args.links_lib) if args.links_lib else e
    try:
        for name, s, mf in (("late", P["S_o_A_frags"], 1), ("contigs_of_8", chopped(P, 8), 1), ("exploded_min_frags_2", exploded_layout(P), 2)):
            for eng in {id(e): e, id(ref): ref}.values():
                eng.upload_frags(s)
                eng.relabel_contigs()
            ln = attempt(lambda: links_call(ref, mf))
            boot = attempt(lambda: boot_call(e, mf))
            out = {"layout": name, "min_frags": mf, "fragments": int(len(s["id_c"])), "contacts": int(len(P["coo_row"])), "replicates": R,
                   "longest_contig": int(np.max(s["l_cont"])), "end_links_ms": ln, "bootstrap_ms": boot,
                   "end_links_lib": args.links_lib or "this build"}
            if "median" in ln and "median" in boot:
                out["links"] = boot_call(e, mf)
                out["r_link_calls_ms"] = R * ln["median"]
                out["ratio"] = boot["median"] / (R * ln["median"])
            print(json.dumps(out), flush=True)
    finally:
        e.close()
        if ref is not e:
            ref._L.graal_destroy(ref._h)
            ref._h = None


if __name__ == "__main__":
    main()
