"""TEST INFRASTRUCTURE -- numpy restatement of graal_map_windows (graal_amd/csrc/map_windows.h), written from its definition: pixel (p, q)
of the window at (u0, v0) is the sum of the bin-1 matrix M1 over the row ranks [u0 + p bin, u0 + (p + 1) bin) and the column ranks
[v0 + q bin, v0 + (q + 1) bin), both cut to [0, S).  Two ways to M1:
  * windows(name, ...)      block-sums the whole bin-1 matrices of a small case (tests/map_reference.py: observed and
                            expected_from_lambda at one rank per pixel);
  * windows_of(P, state, ...)   prices only the pairs a window holds (sim_reference.sub_records + pair_lambda) and adds only the contacts
                            it holds, for layouts whose bin-1 matrix does not fit.
Not product code."""
import numpy as np

from tests import map_reference as MR
from tests import sim_reference as SR


def pixel_ranks(origin, p, bin, S):
    """The clipped ranks [lo, hi) of pixel p on a side that starts at `origin`."""
    lo = int(origin) + int(p) * int(bin)
    return min(max(lo, 0), S), min(max(lo + int(bin), 0), S)


def block_sum(M1, u0, v0, px_rows, px_cols, bin):
    """The window of the S x S matrix M1 (any dtype numpy sums exactly or in float64)."""
    S = len(M1)
    W = np.zeros((px_rows * bin, px_cols * bin), dtype=M1.dtype)
    r0, r1 = pixel_ranks(u0, 0, px_rows * bin, S)
    c0, c1 = pixel_ranks(v0, 0, px_cols * bin, S)
    if r1 > r0 and c1 > c0:
        W[r0 - u0:r1 - u0, c0 - v0:c1 - v0] = M1[r0:r1, c0:c1]
    return W.reshape(px_rows, bin, px_cols, bin).sum(axis=(1, 3))


def bin1(name):
    """(observed float64, expected float64, terms int64) of a small case at one rank per pixel: S x S, symmetric, zero diagonal."""
    P = MR.case(name)
    S = int(P["init_n_sub_frags"])
    R = MR.reference(name, 4096)
    assert R["bin"] == 1 and R["m"] == S
    return R["observed"].astype(np.float64), R["expected"], R["terms"]


def windows(name, origins, px_rows, px_cols, bin):
    """{observed float32, expected float64, terms int64, residual float64}, each [n_win, px_rows, px_cols], of a small case."""
    O1, E1, N1 = bin1(name)
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    O = np.stack([block_sum(O1, u, v, px_rows, px_cols, bin) for u, v in o])
    E = np.stack([block_sum(E1, u, v, px_rows, px_cols, bin) for u, v in o])
    N = np.stack([block_sum(N1, u, v, px_rows, px_cols, bin) for u, v in o])
    return {"observed": O.astype(np.float32), "expected": E, "terms": N, "residual": MR.residual(O, E)}


def windows_of(P, state, origins, px_rows, px_cols, bin, rows=256):
    """The same dict for any layout, from the window's own pairs and contacts.  terms counts the ordered pairs a != b of a pixel;
    `cis` (bool) marks the pixels that hold a pair of one contig priced away from the trans price (linear: closer than d_max);
    `largest` is the largest single lambda of a pixel (a pair that expects 2^31 or more does not fit the maps' fixed point)."""
    rec = SR.sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], state)
    centre, label, _, lbp = rec
    nfpb = P["mean_squared_frags_per_bin"]
    param = np.asarray(P["param_simu"], dtype=np.float32)
    order = MR.order_of(P["np_sub_frags_id"], state)
    S = len(order)
    rank_of = np.full(int(np.asarray(P["np_sub_frags_id"]).reshape(-1, 4)[:, 3].sum()), -1, dtype=np.int64)
    rank_of[order] = np.arange(S)
    r, c = np.asarray(P["coo_row"], dtype=np.int64), np.asarray(P["coo_col"], dtype=np.int64)
    ra, rb = rank_of[r], rank_of[c]
    keep = (r != c) & (ra >= 0) & (rb >= 0)
    ra, rb, val = ra[keep], rb[keep], np.asarray(P["coo_val"], dtype=np.float64)[keep]
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    shape = (len(o), px_rows, px_cols)
    O, E, N, cis = np.zeros(shape), np.zeros(shape), np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=bool)
    big = np.zeros(shape)
    for w, (u0, v0) in enumerate(o):
        for x, y in ((ra, rb), (rb, ra)):                      # a contact counts for every ordered (a, b) it connects
            p, q = (x - u0) // bin, (y - v0) // bin
            ok = (p >= 0) & (p < px_rows) & (q >= 0) & (q < px_cols)
            np.add.at(O[w], (p[ok], q[ok]), val[ok])
        c0, c1 = pixel_ranks(v0, 0, px_cols * bin, S)
        r0, r1 = pixel_ranks(u0, 0, px_rows * bin, S)
        if c1 <= c0:
            continue
        for s0 in range(r0, r1, rows):
            u, v = np.broadcast_arrays(np.arange(s0, min(s0 + rows, r1))[:, None], np.arange(c0, c1)[None, :])
            u, v = u.ravel(), v.ravel()
            a, b = order[u], order[v]
            lam = np.where(u != v, SR.pair_lambda(rec, a, b, nfpb, param), 0.0)
            near = (u != v) & (label[a] == label[b]) & ((lbp[a] >= 0) | (np.abs(centre[b] - centre[a]).astype(np.float32) < param[5]))
            p, q = (u - u0) // bin, (v - v0) // bin
            key = p * px_cols + q
            count = lambda wt: np.bincount(key, weights=wt, minlength=px_rows * px_cols).reshape(px_rows, px_cols)
            E[w] += count(lam)
            N[w] += count((u != v).astype(np.float64)).astype(np.int64)
            cis[w] |= count(near.astype(np.float64)) > 0
            np.maximum.at(big[w], (p, q), lam)
    return {"observed": O.astype(np.float32), "expected": E, "terms": N, "cis": cis, "largest": big, "residual": MR.residual(O, E), "rank_of_sub": rank_of,
            "order": order}
