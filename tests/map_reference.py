"""TEST INFRASTRUCTURE -- numpy restatement of graal_layout_maps (graal_amd/csrc/maps.h): the genome order and the pixel of every
sub-fragment from a layout, the observed image by np.add.at, the expected image by brute force over every sub-fragment pair
(tests/sim_reference.expected_lambda_matrix prices every pair and clamps at 0), and the residual of the two.  Not product code.
"""
import functools

import numpy as np

from tests import junction_reference as JR
from tests import sim_reference as SR


def order_of(sub_id, state):
    """full_order_high of sampler.display_current_matrix: contigs by ascending label (a contig with an inactive fragment is left out),
    fragments by position, a fragment's sub-fragments in stored order, reversed when ori == -1."""
    sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    idc, pos, ori, act = (np.asarray(state[k]) for k in ("id_c", "pos", "ori", "activ"))
    order = []
    for c in np.unique(idc):
        members = np.nonzero(idc == c)[0]
        if not np.all(act[members] == 1):
            continue
        for f in members[np.argsort(pos[members], kind="stable")]:
            ids = list(sid[f, :sid[f, 3]])
            order.extend(ids[::-1] if ori[f] == -1 else ids)
    return np.array(order, dtype=np.int64)


def shape(S, max_px):
    b = max(1, -(-S // int(max_px)))
    return b, -(-S // b)


def pixels(sub_id, state, max_px):
    """(order, pixel_of_sub int32 [-1: not ranked], bin, m)"""
    sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    order = order_of(sid, state)
    b, m = shape(len(order), max_px)
    pix = np.full(int(sid[:, 3].sum()), -1, dtype=np.int32)
    pix[order] = np.arange(len(order)) // b
    return order, pix, b, m


def observed(row, col, count, pix, m):
    r, c = np.asarray(row), np.asarray(col)
    pr, pc = pix[r].astype(np.int64), pix[c].astype(np.int64)
    keep = (pr >= 0) & (pc >= 0) & (r != c)
    v = np.asarray(count, dtype=np.float64)[keep]
    img = np.zeros(m * m, dtype=np.float64)
    np.add.at(img, pr[keep] * m + pc[keep], v)
    np.add.at(img, pc[keep] * m + pr[keep], v)
    return img.reshape(m, m).astype(np.float32)


def expected_from_lambda(a, b, lam, pix, m):
    """(E float64 [m, m], the number of terms added to every pixel, the sum of all lambda): every pair a < b adds its lambda to
    [p(a), p(b)] and to [p(b), p(a)] -- a diagonal pixel holds twice the pairs inside it, like the observed image."""
    pa, pb = pix[a].astype(np.int64), pix[b].astype(np.int64)
    keep = (pa >= 0) & (pb >= 0)
    pa, pb, lam = pa[keep], pb[keep], lam[keep]
    E = np.zeros(m * m, dtype=np.float64)
    N = np.zeros(m * m, dtype=np.int64)
    for x, y in ((pa, pb), (pb, pa)):
        np.add.at(E, x * m + y, lam)
        np.add.at(N, x * m + y, 1)
    return E.reshape(m, m), N.reshape(m, m), float(lam.sum())


def residual(O, E):
    O, E = np.asarray(O, dtype=np.float64), np.asarray(E, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where(E > 0, (O - E) / np.sqrt(np.where(E > 0, E, 1.0)), 0.0)


# the sizes every case is drawn at: bin 1; a small bin whose pixels straddle fragment boundaries (50 or 100, whichever does); a large bin
# with a ragged last pixel
MAX_PX = {"sub3": (4096, 50, 7), "sub1": (4096, 100, 7), "circ": (4096, 100, 7), "wide": (4096, 50, 7)}


@functools.lru_cache(maxsize=None)
def case(name):
    """junction_reference's cases, and "wide": 240 bins x 3 sub-fragments in 3 contigs whose longest is several windows long."""
    if name != "wide":
        return JR.case(name)
    from graal_amd import synth
    par = synth.make_param_simu(fact=2000.0, v_inter=0.05)
    P = synth.make_problem(n_bins=240, nnz=1500, n_sub=3, seed=24, contig_weights=(5, 3, 2), mean_len_bp=1500.0, accu=("random", 1, 4), param=par)
    s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
    s["ori"][::5] = -1
    P["S_o_A_frags"] = s
    P["param_simu"] = par
    return P


@functools.lru_cache(maxsize=None)
def lambdas(name):
    """(a, b, lambda) of every sub-fragment pair of a case, computed once and shared (read only)."""
    P = case(name)
    a, b, lam = SR.expected_lambda_matrix(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
                                          P["param_simu"], P["S_o_A_frags"])
    for x in (a, b, lam):
        x.setflags(write=False)
    return a, b, lam


@functools.lru_cache(maxsize=None)
def reference(name, max_px):
    """Everything the maps of case `name` at `max_px` should be: a dict (shared, read only)."""
    P = case(name)
    order, pix, b, m = pixels(P["np_sub_frags_id"], P["S_o_A_frags"], max_px)
    O = observed(P["coo_row"], P["coo_col"], P["coo_val"], pix, m)
    E, N, total = expected_from_lambda(*lambdas(name), pix, m)
    return {"order": order, "pixel_of_sub": pix, "bin": b, "m": m, "observed": O, "expected": E, "terms": N, "lambda_sum": total,
            "residual": residual(O, E)}


def window_facts(P):
    """(longest contig in kb, d_max in kb, cis pairs of sub-fragments at or beyond d_max, cis pairs inside it) of a case's linear contigs."""
    centre, label, _, lbp = SR.sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["S_o_A_frags"])
    d_max = float(np.float32(P["param_simu"][5]))
    a, b = np.triu_indices(len(centre), 1)
    cis = (label[a] == label[b]) & (lbp[a] < 0)
    d = np.abs(centre[b] - centre[a])[cis]
    return float(np.max(P["S_o_A_frags"]["l_cont_bp"])) / 1000.0, d_max, int((d >= d_max).sum()), int((d < d_max).sum())
