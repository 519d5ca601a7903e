"""TEST INFRASTRUCTURE -- numpy restatement of graal_layout_maps (graal_amd/csrc/maps.h): the genome order and the pixel of every
sub-fragment from a layout, the observed image by np.add.at, the expected image by brute force over every sub-fragment pair
(tests/sim_reference.expected_lambda_matrix prices every pair and clamps at 0; expected_chunked does the same block by block for layouts
whose pairs do not fit at once), and the residual of the two.  Not product code.
"""
import concurrent.futures
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


def order_and_slots(sub_id, state):
    """(order_of's order, the slot of each of its entries): a slot is a fragment's place in the genome order (contigs by ascending label,
    fragments by position) -- junctions.h's numbering, the unit k_mp_cis tiles by 64."""
    sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    idc, pos, ori, act = (np.asarray(state[k]) for k in ("id_c", "pos", "ori", "activ"))
    order, slots, k = [], [], 0
    for c in np.unique(idc):
        members = np.nonzero(idc == c)[0]
        if not np.all(act[members] == 1):
            continue
        for f in members[np.argsort(pos[members], kind="stable")]:
            ids = list(sid[f, :sid[f, 3]])
            order.extend(ids[::-1] if ori[f] == -1 else ids)
            slots.extend([k] * len(ids))
            k += 1
    return np.array(order, dtype=np.int64), np.array(slots, dtype=np.int64)


def expected_chunked(P, state, max_pxs, far_slots=(), rows=128, threads=4):
    """The brute force of expected_from_lambda without holding every pair at once, for layouts of ~10,000 sub-fragments: walks blocks of
    `rows` ranks u of the genome order, prices every pair (u, v > u) with sim_reference.pair_lambda and adds it to the pixel pair of every
    max_px of `max_pxs` in the same pass.  -> {max_px: {"bin", "m", "expected" float64 [m, m], "terms" int64 [m, m], "far": {d: float64
    [m, m]}}}.  expected and terms are expected_from_lambda's E and N (every pair both ways, a diagonal pixel twice); only the order of
    the float64 additions differs.  far[d], for every d of `far_slots`, is the part of `expected` that only the windowed pass over cis
    pairs at least d slots apart can supply: the sum of lambda - max(trans price, 0) over those pairs (what a kernel that loses the tiles
    of those pairs would leave out; beyond the window it is exactly 0, there the cis price is the trans price)."""
    rec = SR.sub_records(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], state)
    _, label, acc, _ = rec
    nfpb = P["mean_squared_frags_per_bin"]
    param = np.asarray(P["param_simu"], dtype=np.float32)
    order, slot = order_and_slots(P["np_sub_frags_id"], state)
    S = len(order)
    out = {}
    for px in max_pxs:
        b, m = shape(S, px)
        out[px] = {"bin": b, "m": m, "expected": np.zeros((m, m)), "terms": np.zeros((m, m), dtype=np.int64),
                   "far": {d: np.zeros((m, m)) for d in far_slots}}
    shapes = [(r["bin"], r["m"]) for r in out.values()]

    def block(u0):
        """The slabs (rows p0 .. p1 - 1 of the upper triangle) that ranks u0 .. u0 + rows - 1 add to each image."""
        u1 = min(u0 + rows, S)
        u, v = np.broadcast_arrays(np.arange(u0, u1)[:, None], np.arange(u0 + 1, S)[None, :])
        keep = v > u
        u, v = u[keep], v[keep]
        a, b = order[u], order[v]
        lam = SR.pair_lambda(rec, a, b, nfpb, param)
        if far_slots:
            norm = ((acc[a] * acc[b]).astype(np.float32) / np.float32(nfpb)).astype(np.float32)
            excess = np.where(label[a] == label[b], lam - np.maximum((param[7] * norm).astype(np.float32), np.float32(0)).astype(np.float64), 0.0)
            gap = slot[v] - slot[u]
        slabs = []
        for bn, m in shapes:
            p0, p1 = u0 // bn, (u1 - 1) // bn + 1
            key = (u // bn - p0) * m + v // bn                  # (u < v: the upper triangle)
            count = lambda w=None: np.bincount(key, weights=w, minlength=(p1 - p0) * m).reshape(p1 - p0, m)
            slabs.append((p0, p1, count(lam), count(), [count(np.where(gap >= d, excess, 0.0)) for d in far_slots]))
        return slabs

    # (numpy prices a block without the interpreter lock: a few threads; the slabs are added in block order, so the sums do not depend on them)
    with concurrent.futures.ThreadPoolExecutor(max(1, int(threads))) as pool:
        for slabs in pool.map(block, range(0, S - 1, rows)):
            for r, (p0, p1, E, N, far) in zip(out.values(), slabs):
                r["expected"][p0:p1] += E
                r["terms"][p0:p1] += N
                for d, F in zip(far_slots, far):
                    r["far"][d][p0:p1] += F
    for r in out.values():
        r["expected"] = r["expected"] + r["expected"].T       # (a pair inside one pixel lands on the diagonal once: twice now)
        r["terms"] = r["terms"] + r["terms"].T
        r["far"] = {d: F + F.T for d, F in r["far"].items()}
    return out


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
