"""TEST INFRASTRUCTURE -- numpy restatement of graal_junction_gaps (graal_amd/csrc/junction_gaps.h): the likelihood profile of the gap at
every junction.

    G[g][f] = sum over the straddling sub-fragment pairs (a left of the junction behind f, b right, one linear contig) of
              rint(Q * ob * (ln ex_g - ln ex_0)) per contact  -  rint(Q * sum over a fragment pair's sub-fragment pairs of ex_g - ex_0),
    sd = |centre_b - centre_a| (float32), sd_g = float32(sd + gap), ex = float32(rippe(.) * norm), norm = float32(accu_a accu_b / nfpb).

Two restatements of the same definition.  gap_profiles(): brute force over the straddling pairs of every junction, built on
junction_reference.rippe_cr (float64 per operation, rounded to float32) and sim_reference.sub_records -- for the small cases.  Gaps:
vectorised on window_reference.Window (its centres, its cis price, its windowed pair enumeration and the prefix-sum identity) -- for the
1,000-bin genome and the mid-size case; tests/test_junction_gaps_cpu.py holds the two equal word for word on the small cases.
fold(): best / q_best / lo / hi of a profile matrix.  simulated(): the junction tests' 1,000-bin genome with three runs of bins taken
out of contig 0 and the hole closed.  Not product code."""
import numpy as np

from tests import junction_reference as JR
from tests import window_reference as WR
from tests.sim_reference import sub_records

f32 = np.float32
Q = JR.Q
VALID, END, CIRCULAR, NONFINITE = JR.VALID, JR.END, JR.CIRCULAR, JR.NONFINITE
DROP_Q = int(round(1.92 * Q))


def gap_profiles(sub_id, sub_len_kb, sub_accu, nfpb, param, state, row, col, count, gaps):
    """(G int64[len(gaps), n] in Q, status uint8[n], sum of |terms| int64[len(gaps), n] in Q), brute force over the straddling pairs
    of every junction of the layout `state`."""
    centre, label, acc, _ = sub_records(sub_id, sub_len_kb, sub_accu, state)
    sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    n = len(sid)
    bin_of = np.zeros(len(centre), np.int64)
    for b in range(n):
        bin_of[sid[b, :sid[b, 3]]] = b
    nsub = sid[:, 3]
    nfpb = f32(nfpb)
    p = [f32(x) for x in param]
    gaps = [f32(g) for g in gaps]
    ng = len(gaps)
    cache = {}

    def prices(a, b):
        """(ex_0, [ex_g]) of the sub-fragment pair, float32."""
        key = (a, b)
        if key not in cache:
            norm = f32(f32(int(acc[a]) * int(acc[b])) / nfpb)
            sd = f32(abs(f32(centre[b] - centre[a])))
            cache[key] = (f32(JR.rippe_cr(sd, p) * norm), [f32(JR.rippe_cr(f32(sd + g), p) * norm) for g in gaps])
        return cache[key]

    pos = np.asarray(state["pos"]); idc = np.asarray(state["id_c"]); nxt = np.asarray(state["next"]); circ = np.asarray(state["circ"])
    G = np.zeros((ng, n), np.int64)
    A = np.zeros((ng, n), np.int64)
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
        total, absum, bad = [0] * ng, [0] * ng, False
        for r, c, ob in zip(row, col, count):
            br, bc = bin_of[r], bin_of[c]
            if not ((br in left and bc in right) or (br in right and bc in left)):
                continue
            e0, eg = prices(r, c)
            for g in range(ng):
                with np.errstate(all="ignore"):
                    v = ob * (np.log(np.float64(eg[g])) - np.log(np.float64(e0)))
                if not np.isfinite(v):
                    bad = True
                    continue
                t = JR._q(v)
                total[g] += t; absum[g] += abs(t)
        for x in left:
            for y in right:
                accm = [0.0] * ng
                for a in sid[x, :nsub[x]]:
                    for b in sid[y, :nsub[y]]:
                        e0, eg = prices(a, b)
                        for g in range(ng):
                            accm[g] += np.float64(eg[g]) - np.float64(e0)
                for g in range(ng):
                    if not np.isfinite(accm[g]):
                        bad = True
                        continue
                    t = -JR._q(accm[g])
                    total[g] += t; absum[g] += abs(t)
        status[f] = NONFINITE if bad else VALID
        if not bad:
            G[:, f] = total
        A[:, f] = absum
    return G, status, A


def reference(P, gaps, state=None):
    return gap_profiles(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
                        P["param_simu"], P["S_o_A_frags"] if state is None else state, P["coo_row"], P["coo_col"], P["coo_val"], gaps)


class Gaps:
    """The same profile, vectorised.  W: a window_reference.Window (its trans-branch flag plays no part: the pairs stay cis)."""

    def __init__(self, W):
        self.W = W

    def _mass(self, X, Y, CX, CY, gaps):
        W = self.W
        acc = np.zeros((len(gaps), len(X)))
        nx, ny = W.nsub[X], W.nsub[Y]
        for i in range(3):
            for j in range(3):
                k = np.nonzero((i < nx) & (j < ny))[0]
                if len(k) == 0:
                    continue
                aa, ab = W.acc_s[X[k], i], W.acc_s[Y[k], j]
                sd = np.abs(CY[k, j] - CX[k, i]).astype(np.float32)
                e0 = W.cis(aa, ab, sd).astype(np.float64)
                for g, gap in enumerate(gaps):
                    acc[g, k] += W.cis(aa, ab, (sd + f32(gap)).astype(np.float32)).astype(np.float64) - e0
        bad = ~np.isfinite(acc)
        t = np.zeros(acc.shape, np.int64)
        t[~bad] = -np.rint(acc[~bad] * Q).astype(np.int64)
        return t, bad

    def profiles(self, state, gaps):
        """(G int64[len(gaps), n], status uint8[n], sum of |terms| int64[len(gaps), n]), as gap_profiles."""
        W = self.W
        n, ng = W.n, len(gaps)
        gaps = np.asarray(gaps, np.float32)
        idc, pos, circ = (np.asarray(state[k], np.int64) for k in ("id_c", "pos", "circ"))
        fwd = np.asarray(state["ori"]) == 1
        start_bp = np.asarray(state["start_bp"], np.int64)
        len_bp = np.asarray(state["len_bp"], np.int64)
        C = W.centres(np.arange(n), start_bp, fwd)
        br, sr = W._sub(W.row)
        bc, sc = W._sub(W.col)
        same = (idc[br] == idc[bc]) & (br != bc)
        G = np.zeros((ng, n), np.int64)
        A = np.zeros((ng, n), np.int64)
        status = np.full(n, END, np.uint8)
        status[circ == 1] = CIRCULAR
        for lab, m in WR._runs(idc, pos):
            if circ[m[0]] == 1 or len(m) < 2:
                continue
            L = len(m)
            D = np.zeros((ng, L + 1), np.int64)
            Da = np.zeros((ng, L + 1), np.int64)
            Db = np.zeros(L + 1, np.int64)
            terms = []
            for ii, jj, _ in W._window_pairs(start_bp[m], start_bp[m] + len_bp[m]):
                if len(ii):
                    X, Y = m[ii], m[jj]
                    terms.append((ii, jj) + self._mass(X, Y, C[X], C[Y], gaps))
            k = np.nonzero(same & (idc[br] == lab))[0]
            a, b = br[k], bc[k]
            aa, ab = W.acc_s[a, sr[k]], W.acc_s[b, sc[k]]
            sd = np.abs(C[b, sc[k]] - C[a, sr[k]]).astype(np.float32)
            old = W.cis(aa, ab, sd)
            t = np.zeros((ng, len(k)), np.int64)
            bad = np.zeros((ng, len(k)), bool)
            for g, gap in enumerate(gaps):
                t[g], bad[g] = W.contact_terms(W.count[k], W.cis(aa, ab, (sd + gap).astype(np.float32)), old, guard=False)
            terms.append((np.minimum(pos[a], pos[b]), np.maximum(pos[a], pos[b]), t, bad))
            for lo, hi, t, bad in terms:
                anyb = bad.any(axis=0).astype(np.int64)
                np.add.at(Db, lo, anyb); np.add.at(Db, hi, -anyb)
                for g in range(ng):
                    np.add.at(D[g], lo, t[g]); np.add.at(D[g], hi, -t[g])
                    np.add.at(Da[g], lo, np.abs(t[g])); np.add.at(Da[g], hi, -np.abs(t[g]))
            f = m[:L - 1]
            b_ = np.cumsum(Db)[:L - 1]
            status[f] = np.where(b_ > 0, NONFINITE, VALID)
            G[:, f] = np.where(b_ > 0, 0, np.cumsum(D, axis=1)[:, :L - 1])
            A[:, f] = np.cumsum(Da, axis=1)[:, :L - 1]
        return G, status, A


def vectorised(P, gaps, state=None):
    return Gaps(WR.window(P)).profiles(P["S_o_A_frags"] if state is None else state, gaps)


def fold(G, status, drop_q):
    """(best int32[n], q_best int64[n], lo int32[n], hi int32[n]) of the profile matrix G[n_gaps, n]: the first index of the largest
    value, that value, the smallest and the largest index with G >= q_best - drop_q; zeros where the status is not VALID."""
    G = np.asarray(G, np.int64)
    ok = np.asarray(status) == VALID
    best = G.argmax(axis=0)                                  # (the first of equal maxima: the smallest gap)
    qb = G.max(axis=0)
    inside = G >= (qb - int(drop_q))[None, :]
    lo = inside.argmax(axis=0)
    hi = G.shape[0] - 1 - inside[::-1].argmax(axis=0)
    z = lambda v, t: np.where(ok, v, 0).astype(t)
    return z(best, np.int32), z(qb, np.int64), z(lo, np.int32), z(hi, np.int32)


# ---- the cases the CPU and GPU tests share ------------------------------------------------------------------------------------------
_CACHE = {}


def small_grid(P):
    """11 values for a small case: 0, three below one sub-fragment length, five that carry some straddling pairs across d_max and not
    others (fractions of d_max: a pair d apart crosses once the gap reaches d_max - d), and two >= d_max (d_max itself among them)."""
    d_max = float(f32(P["param_simu"][5]))
    sub = np.asarray(P["np_sub_frags_len_bp"], np.float32).reshape(-1, 3)
    shortest = float(sub[sub > 0].min())
    g = np.array([0.0, 0.1 * shortest, 0.5 * shortest, 0.9 * shortest, 0.02 * d_max, 0.1 * d_max, 0.3 * d_max, 0.6 * d_max, 0.9 * d_max,
                  d_max, 1.5 * d_max], np.float32)
    g[-2] = f32(P["param_simu"][5])
    assert (np.diff(g) > 0).all(), g
    return g


def wide_grid(P):
    """19 values: small_grid's 11 and 8 geometric ones between them, up to 2 d_max."""
    d_max = float(f32(P["param_simu"][5]))
    g = np.unique(np.concatenate([small_grid(P), np.geomspace(0.003 * d_max, 2.0 * d_max, 8).astype(np.float32)]))
    assert len(g) == 19
    return g


def small(name):
    """(P, grid, G, status, A) of junction_reference.case(name) on small_grid, by the brute-force restatement."""
    if name not in _CACHE:
        P = JR.case(name)
        g = small_grid(P)
        _CACHE[name] = (P, g) + reference(P, g)
    return _CACHE[name]


PLANTED = ((200, 3), (300, 10), (400, 30))                  # (position in contig 0 of the last bin kept, bins removed behind it)
STAT_GRID = np.concatenate([[0.0], np.geomspace(0.5, 400.0, 40)]).astype(np.float32)


def simulated():
    """The 1,000-bin genome of tests/test_junctions_gpu.py (fact 300, v_inter 0.02, seed 11).  -> (P, true layout, test layout, planted):
    the test layout has the PLANTED runs of contig 0 in contigs of their own and the hole closed; planted = [(fragment before the
    hole, true gap in kb)]."""
    if "sim" not in _CACHE:
        from graal_amd import synth
        from tests.test_junctions_gpu import _layout
        par = synth.make_param_simu(fact=300.0, v_inter=0.02)
        P = synth.make_problem(n_bins=1000, nnz=500, n_sub=1, seed=11, contig_weights=(5, 3, 2), param=par)
        P["param_simu"] = par
        s = {k: np.asarray(v) for k, v in P["S_o_A_frags"].items()}
        contigs = []
        for cid in np.unique(s["id_c"]):
            m = np.nonzero(s["id_c"] == cid)[0]
            contigs.append([(int(f), int(s["ori"][f])) for f in m[np.argsort(s["pos"][m])]])
        c0, keep, runs, planted, at = contigs[0], [], [], [], 0
        for p, k in PLANTED:
            keep += c0[at:p + 1]
            runs.append(c0[p + 1:p + 1 + k])
            planted.append((c0[p][0], float(sum(int(s["len_bp"][f]) for f, _ in runs[-1])) / 1000.0))
            at = p + 1 + k
        keep += c0[at:]
        _CACHE["sim"] = (P, s, _layout(s["len_bp"], [keep] + contigs[1:] + runs), planted)
    return _CACHE["sim"]


def check_simulated(G, status, state, planted, drop_q=DROP_Q):
    """The two conditions on simulated data: every planted gap inside [lo, hi], and the share of the other valid junctions with grid
    index 0 inside theirs.  -> (inside bool per planted gap, that share, [(gap, best, lo, hi in kb)])."""
    best, qb, lo, hi = fold(G, status, drop_q)
    ok = np.asarray(status) == VALID
    inside, rows = [], []
    for f, gap in planted:
        assert ok[f]
        inside.append(bool(STAT_GRID[lo[f]] <= gap <= STAT_GRID[hi[f]]))
        rows.append((gap, float(STAT_GRID[best[f]]), float(STAT_GRID[lo[f]]), float(STAT_GRID[hi[f]])))
    others = ok.copy()
    others[[f for f, _ in planted]] = False
    return inside, float((lo[others] == 0).mean()), rows
