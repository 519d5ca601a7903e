"""TEST INFRASTRUCTURE -- numpy restatement of graal_junction_bootstrap (graal_amd/csrc/junction_boot.h): the Poisson bootstrap of the
contacts behind every junction score.  Built on tests/sim_reference.py (the Philox counters, the uniform stream, the Poisson sampler and
its near-a-boundary flag), on tests/window_reference.py (the contact model's prices, the mass part M by its vectorised junction scores on
an empty contact list) and, for its own check, on tests/junction_reference.py (tests/test_junction_bootstrap_cpu.py: with the draw
replaced by the count itself it is junction_scores exactly).

    J*_r[f] = M[f] + sum over the contacts k straddling the junction behind f of rint(Q * draw_{k,r} * (ln ex_cis,k - ln ex_trans,k)),
    draw_{k,r} = poisson(ob_k, Stream(row_k, col_k, 2 | r << 8, seed)).

A draw whose uniform came within 1e-6 (relative) of a boundary it was compared with is FLAGGED (Stream.near): the GPU's exp / ln round
differently from libm in the last place and may tip it.  A flagged draw excuses the (junction, replicate) cells it straddles, nothing else.
Counts below 10 (inversion) are drawn vectorised with the scalar sampler's operations in its order; counts of 10 and more go through
sim_reference.poisson itself.  A contact whose unit term is exactly 0 (beyond the window: cis and trans are the same float32) draws
nothing on the GPU and flags nothing here.  Not product code."""
import copy
import math

import numpy as np

from tests import sim_reference as SR
from tests import window_reference as WR

Q = WR.Q
VALID = WR.J_VALID


def draw_counts(row, col, ob, seed, r):
    """(count int64[m], flagged bool[m]): poisson(ob, Stream(row, col, 2 | r << 8, seed)) per contact."""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    lam = np.asarray(ob, np.float64)
    tag = 2 | (int(r) << 8)
    out = np.zeros(len(lam), np.int64)
    flag = np.zeros(len(lam), bool)
    idx = np.nonzero((lam > 0.0) & (lam < SR.PTRS_MIN))[0]
    if len(idx):
        # sim_reference._inversion, vectorised: one uniform, F compared (and flagged) at every k it reaches
        u, _ = SR.uniforms_from_words(SR.philox4x32(row[idx], col[idx], tag, 0, seed))
        l = lam[idx]
        p = np.array([math.exp(-x) for x in l])
        F = p.copy()
        k = np.zeros(len(l), np.int64)

        def near(a, b):
            return np.abs(a - b) <= SR.TOL * np.maximum(np.abs(a), np.abs(b))
        fl = near(u, F)
        act = u > F
        while act.any():
            k[act] += 1
            p[act] = p[act] * l[act] / k[act].astype(np.float64)
            F[act] = F[act] + p[act]
            fl[act] |= near(u[act], F[act])
            act = act & (u > F) & (k < SR.KMAX)
        out[idx] = k
        flag[idx] = fl
    for i in np.nonzero(lam >= SR.PTRS_MIN)[0]:
        st = SR.Stream(row[i], col[i], tag, seed)
        out[i] = SR.poisson(float(lam[i]), st)
        flag[i] = st.flag
    return out, flag


class Boot:
    """The junctions of one layout of one problem: M, the statuses and every straddling contact's unit term, once; replicates on demand.
    W: a window_reference.Window (its quirk flag is the mode)."""

    def __init__(self, W, state):
        self.W = W
        n = self.n = W.n
        idc, pos, circ = (np.asarray(state[k], np.int64) for k in ("id_c", "pos", "circ"))
        fwd = np.asarray(state["ori"]) == 1
        # the mass part: the same junctions on an empty contact list
        Wm = copy.copy(W)
        Wm.row = Wm.col = np.zeros(0, np.int64)
        Wm.count = np.zeros(0, np.float64)
        self.M, self.status, self.A_mass = Wm.junction_scores(state)
        # slots: contigs by label, fragments by position (any numbering that keeps a contig's fragments consecutive in position order)
        order = np.lexsort((pos, idc))
        self.slot = np.zeros(n, np.int64)
        self.slot[order] = np.arange(n)
        # the straddling contacts and their unit terms
        C = W.centres(np.arange(n), np.asarray(state["start_bp"], np.int64), fwd)
        br, sr = W._sub(W.row)
        bc, sc = W._sub(W.col)
        k = np.nonzero((idc[br] == idc[bc]) & (br != bc) & (circ[br] == 0))[0]
        a, b = br[k], bc[k]
        aa, ab = W.acc_s[a, sr[k]], W.acc_s[b, sc[k]]
        new = W.cis(aa, ab, np.abs(C[b, sc[k]] - C[a, sr[k]]).astype(np.float32))
        old = W.trans(a, b, aa, ab, fwd[a], fwd[b])
        with np.errstate(all="ignore"):
            t = np.log(new.astype(np.float64)) - np.log(old.astype(np.float64))
        keep = t != 0.0                                     # (NaN != 0: a non-finite unit stays, and marks its junctions)
        self.k, self.t = k[keep], t[keep]
        self.row, self.col, self.ob = W.row[self.k], W.col[self.k], W.count[self.k]
        self.lo = np.minimum(self.slot[a], self.slot[b])[keep]
        self.hi = np.maximum(self.slot[a], self.slot[b])[keep]

    def straddle(self, values, select=None):
        """int64[n] per fragment: the sum of `values` (one per straddling contact, or those in `select`) over the contacts that
        straddle the junction behind it; 0 where the fragment has no valid junction."""
        lo, hi, v = self.lo, self.hi, np.asarray(values)
        if select is not None:
            lo, hi, v = lo[select], hi[select], v[select]
        D = np.zeros(self.n + 1, np.int64)
        np.add.at(D, lo, v.astype(np.int64))
        np.add.at(D, hi, -v.astype(np.int64))
        out = np.cumsum(D)[self.slot]
        return np.where(self.status == VALID, out, 0)

    def terms(self, counts):
        """(term in Q int64[m], non-finite bool[m]) of the straddling contacts under the counts given."""
        with np.errstate(all="ignore"):
            v = np.asarray(counts, np.float64) * self.t
        bad = ~np.isfinite(v)
        q = np.zeros(len(v), np.int64)
        q[~bad] = np.rint(v[~bad] * Q).astype(np.int64)
        return q, bad

    def score(self, counts):
        """(J int64[n], sum of |terms| int64[n], non-finite bool[n]) with the straddling contacts counting `counts`."""
        q, bad = self.terms(counts)
        nf = self.straddle(bad.astype(np.int64)) > 0
        ok = (self.status == VALID) & ~nf
        J = np.where(ok, self.M + self.straddle(q), 0)
        return J, self.A_mass + self.straddle(np.abs(q)), nf

    def replicate(self, seed, r):
        """(J*_r int64[n], sum of |terms| int64[n], flagged bool[n], non-finite bool[n]) of replicate r."""
        c, fl = draw_counts(self.row, self.col, self.ob, seed, r)
        J, A, nf = self.score(c)
        return J, A, self.straddle(fl.astype(np.int64)) > 0, nf

    def replicates(self, seed, reps):
        """The same stacked over the replicates `reps`: four arrays [len(reps), n]."""
        out = [self.replicate(seed, r) for r in reps]
        return tuple(np.stack([o[i] for o in out]) for i in range(4))


def boot(P, state=None, quirk=False):
    return Boot(WR.window(P, quirk), P["S_o_A_frags"] if state is None else state)


# ---- the cases the CPU and GPU tests share ------------------------------------------------------------------------------------------
SMALL_CASES = (("sub3", False, 7), ("sub3", True, 7), ("sub1", False, 8), ("circ", False, 9))     # (junction_reference.case, quirk, seed)
N_REP = 150                             # three batches of the engine's 64, the last one short
REF_REPS = tuple(range(12)) + (63, 64, 127, 128, 149)          # restated: the first ones and both sides of every batch boundary
PLANTED = (25.0, 60.0, 120.0, 250.0, 400.0, 33.0)               # counts for the sampler's branch above 10
FILL = 1.7                              # a non-integer count (a blacklist fill): the rate as it stands, float32(1.7)
MID_SEED, MID_REPS = 12, 4
_CACHE = {}


def small_case(name):
    """junction_reference.case(name) with float32 counts, six of them replaced by PLANTED and one by FILL, each on a contact that
    straddles at least three junctions."""
    if name not in _CACHE:
        from tests import junction_reference as JR
        P = JR.case(name)
        B = boot(P)
        wide = B.k[(B.hi - B.lo >= 3) & np.isfinite(B.t)]
        assert len(wide) >= len(PLANTED) + 1, len(wide)
        pick = wide[np.linspace(0, len(wide) - 1, len(PLANTED) + 1).astype(int)]
        assert len(set(pick.tolist())) == len(pick)
        v = np.asarray(P["coo_val"]).astype(np.float32)
        v[pick[:-1]] = PLANTED
        v[pick[-1]] = FILL
        P["coo_val"] = v
        _CACHE[name] = P
    return _CACHE[name]


def small_boot(name, quirk):
    key = (name, quirk)
    if key not in _CACHE:
        _CACHE[key] = boot(small_case(name), quirk=quirk)
    return _CACHE[key]


def small_replicates(name, quirk, seed):
    key = (name, quirk, seed)
    if key not in _CACHE:
        _CACHE[key] = small_boot(name, quirk).replicates(seed, REF_REPS)
    return _CACHE[key]


def mid_case():
    """window_cases.m2 without its last contact: 119,999 contacts, so that the list does not end on a wave's 64."""
    if "m2" not in _CACHE:
        from tests import window_cases as WC
        P = dict(WC.m2())
        for k in ("coo_row", "coo_col", "coo_val"):
            P[k] = np.asarray(P[k])[:-1]
        _CACHE["m2"] = P
    return _CACHE["m2"]


def mid_replicates(quirk, state=None):
    """(Boot, its MID_REPS replicates under MID_SEED) of mid_case() in the layout `state` (its own by default)."""
    key = ("m2", quirk, None if state is None else np.asarray(state["id_c"]).tobytes())
    if key not in _CACHE:
        B = boot(mid_case(), state, quirk)
        _CACHE[key] = (B, B.replicates(MID_SEED, range(MID_REPS)))
    return _CACHE[key]
