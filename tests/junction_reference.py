"""TEST INFRASTRUCTURE -- numpy restatement of graal_junction_scores (graal_amd/csrc/junctions.h), by brute force over the straddling pairs
of every junction.  The contact model is evaluated operation by operation in float64 and rounded to float32 after each one, as the engine's
correctly rounded float32 model (model_math.h) does; a term is rounded to Q = 2^30 once (a contact; a fragment pair's mass).  Not product code.
"""
import numpy as np

from tests.sim_reference import sub_records

f32 = np.float32
Q = float(1 << 30)
VALID, END, CIRCULAR, NONFINITE = 0, 1, 2, 3


def rippe_cr(s, p):
    """rippe (graal_hip.hip) with correctly rounded powf / expf: float64 per operation, rounded to float32."""
    kuhn, lm, c1, slope, d, d_max, fact, v = [f32(x) for x in p]
    s = f32(s)
    r = f32(0)
    if s > 0 and s < d_max:
        n = f32(s * lm)
        if kuhn != f32(1):
            n = f32(n / kuhn)
        inner = f32(f32(n * n) + d)
        e = f32(np.exp(np.float64(f32(f32(d - f32(2)) / inner))))
        pw = f32(np.float64(s) ** np.float64(slope))
        r = f32(f32(f32(c1 * pw) * e) * fact)
    return max(r, v)


def _q(v):
    return int(np.rint(v * Q))


def junction_scores(sub_id, sub_len_kb, sub_accu, nfpb, param, state, row, col, count, quirk=False):
    """(J int64[n] in Q, status uint8[n], sum of |terms| int64[n] in Q) for the layout `state` (linear contigs only are scored)."""
    centre, label, acc, _ = sub_records(sub_id, sub_len_kb, sub_accu, state)
    sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    n = len(sid)
    bin_of = np.zeros(len(centre), np.int64)
    for b in range(n):
        bin_of[sid[b, :sid[b, 3]]] = b
    fwd = np.asarray(state["ori"]) == 1
    nsub = sid[:, 3]
    last_acc = np.array([acc[sid[b, nsub[b] - 1]] for b in range(n)])
    nfpb = f32(nfpb)
    p = [f32(x) for x in param]
    v_inter = p[7]

    def trans(a, b):
        aa, ab = int(acc[a]), int(acc[b])
        ba, bb = bin_of[a], bin_of[b]
        if quirk:
            if ba < bb:
                if not fwd[ba]:
                    aa = int(last_acc[ba])
            elif not fwd[bb]:
                ab = int(last_acc[bb])
        return f32(v_inter * f32(f32(aa * ab) / nfpb))

    cache = {}

    def cis(a, b):
        key = (a, b)
        if key not in cache:
            cache[key] = _cis(a, b)
        return cache[key]

    def _cis(a, b):
        norm = f32(f32(int(acc[a]) * int(acc[b])) / nfpb)
        return f32(rippe_cr(abs(f32(centre[b] - centre[a])), p) * norm)

    pos = np.asarray(state["pos"]); idc = np.asarray(state["id_c"]); nxt = np.asarray(state["next"]); circ = np.asarray(state["circ"])
    J = np.zeros(n, np.int64)
    A = np.zeros(n, np.int64)
    status = np.full(n, END, np.uint8)
    row, col, count = np.asarray(row), np.asarray(col), np.asarray(count, dtype=np.float64)
    for f in range(n):
        if circ[f] == 1:
            status[f] = CIRCULAR
            continue
        if nxt[f] == -1:
            continue
        members = np.nonzero(idc == idc[f])[0]
        left = set(members[pos[members] <= pos[f]].tolist())
        right = set(members[pos[members] > pos[f]].tolist())
        total, absum, bad = 0, 0, False
        for r, c, ob in zip(row, col, count):
            br, bc = bin_of[r], bin_of[c]
            if not ((br in left and bc in right) or (br in right and bc in left)):
                continue
            with np.errstate(all="ignore"):
                v = ob * (np.log(np.float64(cis(r, c))) - np.log(np.float64(trans(r, c))))
            if not np.isfinite(v):
                bad = True
                continue
            t = _q(v)
            total += t; absum += abs(t)
        for x in left:
            for y in right:
                accm = 0.0
                for a in sid[x, :nsub[x]]:
                    for b in sid[y, :nsub[y]]:
                        accm += np.float64(cis(a, b)) - np.float64(trans(a, b))
                if not np.isfinite(accm):
                    bad = True
                    continue
                t = -_q(accm)
                total += t; absum += abs(t)
        status[f] = NONFINITE if bad else VALID
        J[f] = total if not bad else 0
        A[f] = absum
    return J, status, A


def cut_layout(state, f, recentre=True):
    """The layout `state` (a dict of the engine's fields) cut between f and next[f]: the right part becomes a new contig (label max + 1)
    starting at 0 bp, in the same orientation.  recentre=False keeps the right part's coordinates (not a valid layout for the engine, but
    the sparse scorer prices it with the old float32 centres: the cut without re-centring noise)."""
    s = {k: np.array(v, dtype=np.int32, copy=True) for k, v in state.items()}
    c = s["id_c"][f]
    members = np.nonzero(s["id_c"] == c)[0]
    members = members[np.argsort(s["pos"][members])]
    k = int(s["pos"][f]) + 1
    L, R = members[:k], members[k:]
    new = int(s["id_c"].max()) + 1
    shift = int(s["start_bp"][R[0]])
    lbp_l = int(s["len_bp"][L].sum()); lbp_r = int(s["len_bp"][R].sum())
    s["next"][L[-1]] = -1
    s["prev"][R[0]] = -1
    s["id_c"][R] = new
    s["pos"][R] -= k
    if recentre:
        s["start_bp"][R] -= shift
    s["l_cont"][L] = len(L); s["l_cont"][R] = len(R)
    s["l_cont_bp"][L] = lbp_l; s["l_cont_bp"][R] = lbp_r
    return s


def case(name):
    """Small problems with contacts: n_sub 3 with reversed bins and RF counts 1..4, n_sub 1, and a circular contig with RF count 9."""
    from graal_amd import synth
    par = synth.make_param_simu(fact=2000.0, v_inter=0.05)
    if name == "sub3":
        P = synth.make_problem(n_bins=48, nnz=400, n_sub=3, seed=21, contig_weights=(5, 3, 2), mean_len_bp=1500.0, accu=("random", 1, 4), param=par)
        s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
        s["ori"][::4] = -1
    elif name == "sub1":
        P = synth.make_problem(n_bins=120, nnz=600, n_sub=1, seed=22, contig_weights=(4, 3, 3), param=par)
        s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
        s["ori"][1::3] = -1
    else:
        P = synth.make_problem(n_bins=45, nnz=400, n_sub=3, seed=23, contig_weights=(2, 1), mean_len_bp=1500.0, accu=9, param=par)
        s = {k: np.array(v) for k, v in P["S_o_A_frags"].items()}
        s["circ"][s["id_c"] == s["id_c"].min()] = 1
    P["S_o_A_frags"] = s
    P["param_simu"] = par
    return P


def reference(P, state=None, quirk=False):
    return junction_scores(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
                           P["param_simu"], P["S_o_A_frags"] if state is None else state, P["coo_row"], P["coo_col"], P["coo_val"], quirk=quirk)
