"""Hi-C contacts simulated from a known genome under the contact model the engine scores (graal_simulate_contacts, HIP on the GPU).

The GRAAL paper checks its sampler this way: contacts drawn from a known genome under the Rippe model, then scaffolded again.  The
reference's kernel for it (simulate_data_2d, kernels3.cu:2331-2800) sits behind a host wrapper that cannot be called
(cuda_lib_gl.py:1355 vs simulation_loader.py:120); here it is one engine call.  Every sub-fragment pair a < b gets an independent
Poisson count whose mean is the expected value the full likelihood gives that sub-pixel, so at the true layout and the true parameters the
data are what the model says they are.

    simulate_problem(problem, seed, param=None)   -- a synth / pyramid problem dict with all its contact data replaced
    python -m graal_amd.simulate --dataset DIR --seed S --out DIR2 [--param kuhn lm c1 slope d d_max fact v_inter]
        simulates at restriction-fragment resolution from DIR's layout and writes the 3-file dataset DIR2, which
        ``python -m graal_amd.run --dataset DIR2 --size-pyramid 1 --level 0`` scaffolds (reporting the distance to that layout).
"""
import argparse
import sys

import numpy as np

from . import synth
from .lib import Engine


def simulate_contacts(problem, seed, param=None, device=0):
    """(row, col, count) drawn on the GPU from the problem's layout (S_o_A_frags), sub-fragment tables and parameters."""
    par = np.asarray(problem["param_simu"] if param is None else param, dtype=np.float32).reshape(8)
    e = Engine(device)
    try:
        e.upload_subfrags(problem["np_sub_frags_id"], problem["np_sub_frags_len_bp"], problem["np_sub_frags_accu"],
                          problem["init_n_sub_frags"], problem["mean_squared_frags_per_bin"])
        e.set_params(par)
        e.upload_frags(problem["S_o_A_frags"])
        return e.simulate_contacts(seed)
    finally:
        e.close()


def _bin_list(row, col, val, bin_of_sub, n_bins):
    """The bin-level upper COO list (the neighbour proposal's matrix, cuda_lib_gl.py:2363-2390), as synth.make_problem builds it."""
    bi, bj = bin_of_sub[row].astype(np.int64), bin_of_sub[col].astype(np.int64)
    m = bi != bj
    keys = np.minimum(bi[m], bj[m]) * n_bins + np.maximum(bi[m], bj[m])
    ub, inv = np.unique(keys, return_inverse=True)
    bval = np.bincount(inv, weights=np.asarray(val)[m].astype(np.float64)).astype(np.float32)
    return (ub // n_bins).astype(np.int32), (ub % n_bins).astype(np.int32), bval


def _is_coo(m):
    return isinstance(m, (tuple, list)) and len(m) == 3


def _like(coo_old, row, col, val):
    """(row, col, val) in the dtypes of the COO triple it replaces."""
    return tuple(np.asarray(x, dtype=np.asarray(o).dtype) for x, o in zip((row, col, val), coo_old))


def simulate_problem(problem, seed, param=None, device=0):
    """A copy of `problem` whose contacts are simulated from its own layout, which stays the known genome G0; `param` (8 floats)
    replaces param_simu.  `problem` is a synth.make_problem dict (dense matrices from synth.with_dense included) or a
    pyramid.simulation_inputs dict, whose contact matrices are COO triples.  Every contact structure the dict carries is rebuilt from
    the simulated list, so a sampler built from the result scores the simulated data:
      * the sub-level list: coo_row / coo_col / coo_val, and hic_matrix (the likelihood's observations) when present;
      * the bin-level list (the neighbour proposal): bin_coo_*, and hic_matrix_sub_sampled when present;
      * mean_value_trans, by the convention of the dict's source (synth.make_problem's, or the reference loader's for a pyramid dict,
        pyramid_sparse.py:1345-1366 restated in graal_amd/pyramid.py).
    Repeated bins are not supported (graal_simulate_contacts refuses them)."""
    p = dict(problem)
    if int(len(np.asarray(p["S_o_A_frags"]["id_c"]))) != int(p["n_frags"]) or len(p.get("id_frag_duplicated") or []):
        raise ValueError("simulate_problem: problems with repeated bins are not supported")
    if param is not None:
        p["param_simu"] = np.asarray(param, dtype=np.float32).reshape(8)
    row, col, cnt = simulate_contacts(p, seed, device=device)
    p["coo_row"], p["coo_col"], p["coo_val"] = row, col, cnt
    sub_id = np.asarray(p["np_sub_frags_id"]).reshape(-1, 4)
    n_bins, S = len(sub_id), int(p["init_n_sub_frags"])
    bin_of_sub = np.zeros(S, np.int64)
    for k in range(3):
        m = sub_id[:, 3] > k
        bin_of_sub[sub_id[m, k]] = np.nonzero(m)[0]
    brow, bcol, bval = _bin_list(row, col, cnt, bin_of_sub, n_bins)
    p["bin_coo_row"], p["bin_coo_col"], p["bin_coo_val"] = brow, bcol, bval
    p["bin_of_sub"] = bin_of_sub.astype(np.int32)
    id_c = np.asarray(p["S_o_A_frags"]["id_c"])[bin_of_sub]
    trans = id_c[row] != id_c[col]
    n_per_contig = np.unique(id_c, return_counts=True)[1].astype(np.int64)
    pyramid_dict = _is_coo(problem.get("hic_matrix"))
    if pyramid_dict:
        # the reference loader's: the stored (upper) trans sum over sub-fragment pairs of different contigs, float32 divisor
        n_tot = int((n_per_contig * S).sum() - (n_per_contig * n_per_contig).sum())
        p["mean_value_trans"] = np.float64(int(cnt[trans].sum())) / np.float64(np.float32(n_tot)) if n_tot else np.float64(0)
        p["hic_matrix"] = _like(problem["hic_matrix"], row, col, cnt)
        if _is_coo(problem.get("hic_matrix_sub_sampled")):
            p["hic_matrix_sub_sampled"] = _like(problem["hic_matrix_sub_sampled"], brow, bcol, bval)
        else:
            p["hic_matrix_sub_sampled"] = (brow, bcol, bval)
    else:
        n_trans_pairs = float(S) * S - float((n_per_contig.astype(np.float64) ** 2).sum())
        p["mean_value_trans"] = np.float32(2.0 * cnt[trans].sum() / max(n_trans_pairs, 1.0))
        if "hic_matrix" in problem or "hic_matrix_sub_sampled" in problem:
            p = synth.with_dense(p)
    return p


def problem_from_dataset(folder):
    """The level-0 problem of a 3-file dataset (bins = restriction fragments), with the layout of its fragment list."""
    from . import pyramid as pyr
    P = pyr.build_and_filter(folder, 1, 3)
    inp = pyr.simulation_inputs(P, 0)
    n = int(inp["n_frags"])
    return dict(S_o_A_frags=inp["S_o_A_frags"], n_frags=n, init_n_sub_frags=int(inp["init_n_sub_frags"]),
                np_sub_frags_id=inp["np_sub_frags_id"], np_sub_frags_len_bp=inp["np_sub_frags_len_bp"],
                np_sub_frags_accu=inp["np_sub_frags_accu"], mean_squared_frags_per_bin=inp["mean_squared_frags_per_bin"])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dataset", required=True, help="3-file dataset whose fragment layout is the genome to simulate from")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--out", required=True, help="folder of the simulated 3-file dataset")
    ap.add_argument("--param", type=float, nargs=8, default=None,
                    help="kuhn lm c1 slope d d_max fact v_inter (default: synth.make_param_simu())")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    P = problem_from_dataset(args.dataset)
    param = np.asarray(args.param if args.param is not None else synth.make_param_simu(), dtype=np.float32)
    P["param_simu"] = param
    Q = simulate_problem(P, args.seed, device=args.device)
    reads = synth.write_dataset(Q, args.out)
    print("graal_amd.simulate: %d fragments, %d contacts (%d reads) from seed %d -> %s"
          % (Q["n_frags"], len(Q["coo_val"]), reads, args.seed, args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
