"""graal_simulate_contacts on the C5 layout (bench.py's 50,000-fragment stand-in, make_param_simu() defaults).

    python tools/sim_c5.py [--reps N]              one JSON line: contacts, Σcount, wall ms per simulation incl. the copy to the host
    rocprofv3 --kernel-trace --stats -d D -o sim -- python tools/sim_c5.py --reps 3
    python tools/sim_c5.py --summarize D/.../sim_results.db     per-kernel table (Markdown) of such a trace -> profiles/simulate_c5_kernels.md
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(reps):
    from graal_amd import synth
    from graal_amd.lib import Engine
    par = synth.make_param_simu()
    P = synth.make_problem(n_bins=50000, nnz=1000, n_sub=1, seed=20141217, param=par)
    e = Engine(0)
    try:
        e.upload_subfrags(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["init_n_sub_frags"],
                          P["mean_squared_frags_per_bin"])
        e.set_params(par)
        e.upload_frags(P["S_o_A_frags"])
        r, c, v = e.simulate_contacts(2016)           # (warm-up: allocations)
        ms = []
        for i in range(reps):
            t0 = time.perf_counter()
            r, c, v = e.simulate_contacts(2016 + i)
            ms.append(1e3 * (time.perf_counter() - t0))
    finally:
        e.close()
    print(json.dumps({"workload": "C5 layout, 50000 fragments, n_sub 1, make_param_simu()", "d_max_kb": float(par[5]),
                      "contacts": int(len(v)), "sum_count": int(v.sum(dtype="int64")), "reps": reps,
                      "ms_per_simulation_incl_d2h": {"min": min(ms), "median": sorted(ms)[len(ms) // 2], "max": max(ms)}}))


def summarize(db):
    import sqlite3
    con = sqlite3.connect(db)
    rows = con.execute("select name, duration from kernels").fetchall()
    by = {}
    for name, d in rows:
        short = name.replace("(anonymous namespace)::", "").replace("void ", "", 1)
        short = short.split("(")[0] if short.startswith("k_") else short[:110]
        by.setdefault(short, []).append(d / 1e3)
    print("| kernel | launches | median µs | min µs | max µs |\n|---|---|---|---|---|")
    for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1])):
        v = sorted(v)
        print("| `%s` | %d | %.1f | %.1f | %.1f |" % (k, len(v), v[len(v) // 2], v[0], v[-1]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--summarize", default=None)
    a = ap.parse_args()
    summarize(a.summarize) if a.summarize else run(a.reps)
