"""TEST INFRASTRUCTURE -- numpy restatements of graal_block_swaps (graal_amd/csrc/swaps.h).  swap_layout() writes the layout with two
adjacent runs X, Y of a contig swapped (Y first, inside the same bp interval).  Restatement (brute force, in the style of
tests/flip_reference.py) builds that layout per swap and re-prices every sub-fragment pair whose price can change with the correctly
rounded float32 model: X x Y, X x rest of the contig, Y x rest of the contig (cis in both layouts; orientation does not change, so the
trans-branch indexing plays no part).  Window (on tests/window_reference.py's pricing, mass and contact-term helpers) gives the same
numbers for problems of ~10^4 fragments by enumerating a fragment pair's mass only where one of its two gaps is inside the window.  A
term is rounded to Q once (a contact; a fragment pair's mass, the moved run's fragment outer, X's for X x Y).  Per swap: (q, contacts,
status, A), A the sum of |terms| in Q.  No engine record, slot numbering or kernel output.  Not product code.
"""
import numpy as np

from tests import flip_reference as FR
from tests import link_reference as LR
from tests import window_reference as WR
from tests.sim_reference import sub_records

f32 = np.float32
Q = LR.Q
VALID, CIRCULAR, NONFINITE = 0, 1, 2


def _members(state, f, m_, l):
    """(the contig's fragments in position order, X's slice of them, Y's slice)."""
    idc, pos = np.asarray(state["id_c"]), np.asarray(state["pos"])
    assert idc[f] == idc[m_] == idc[l] and pos[f] <= pos[m_] < pos[l]
    m = np.nonzero(idc == idc[f])[0]
    m = m[np.argsort(pos[m])]
    return m, slice(int(pos[f]), int(pos[m_]) + 1), slice(int(pos[m_]) + 1, int(pos[l]) + 1)


def swap_layout(state, first, mid, last):
    """The layout with, for every swap (scalars: one swap), the runs X = first .. mid and Y = behind mid .. last exchanged: Y comes
    first, then X, inside the same bp interval; X's fragments get start_bp + len_bp(Y) and pos + |Y|, Y's start_bp - len_bp(X) and
    pos - |X|; ori is unchanged; prev / next follow."""
    s = {k: np.array(v, dtype=np.int32, copy=True) for k, v in state.items()}
    touched = set()
    start, ln, pos = (np.asarray(state[k]) for k in ("start_bp", "len_bp", "pos"))
    for f, m_, l in zip(np.atleast_1d(first), np.atleast_1d(mid), np.atleast_1d(last)):
        m, sx, sy = _members(state, int(f), int(m_), int(l))
        X, Y = m[sx], m[sy]
        assert not (touched & set(X.tolist() + Y.tolist())), "spans overlap"
        touched |= set(X.tolist() + Y.tolist())
        lx, ly = int(ln[X].sum()), int(ln[Y].sum())
        s["start_bp"][X] = start[X] + ly; s["pos"][X] = pos[X] + len(Y)
        s["start_bp"][Y] = start[Y] - lx; s["pos"][Y] = pos[Y] - len(X)
    circ = np.asarray(s["circ"])
    for c, m in LR.contigs_of(s).items():                             # prev / next along the new position order
        ring = circ[m[0]] == 1 and len(m) > 1
        s["prev"][m] = np.concatenate([[m[-1] if ring else -1], m[:-1]])
        s["next"][m] = np.concatenate([m[1:], [m[0] if ring else -1]])
        if circ[m[0]] == 1 and len(m) == 1:
            s["prev"][m] = state["prev"][m]; s["next"][m] = state["next"][m]
    return s


def swapped_back(state, first, mid, last):
    """(first, mid, last) that name, in swap_layout(state, first, mid, last), the swaps that undo it: Y's first, Y's last, X's last."""
    nx = np.asarray(state["next"])
    return nx[np.atleast_1d(mid)], np.atleast_1d(last), np.atleast_1d(mid)


class Restatement(LR.Restatement):
    """swaps(state, first, mid, last) restates graal_block_swaps by brute force, one swap at a time."""

    def new_layout(self, state, f, m_, l):
        return swap_layout(state, f, m_, l)

    def groups(self, X, Y, R_):
        """(outer bins, inner bins) of the fragment pairs whose price changes."""
        return [(X, Y), (X, R_), (Y, R_)]

    def swaps(self, state, first, mid, last):
        out = [self._swap(state, int(f), int(m_), int(l)) for f, m_, l in zip(first, mid, last)]
        q, c, st, A = (np.array(x) for x in zip(*out)) if out else ([], [], [], [])
        return np.asarray(q, np.int64), np.asarray(c, np.int64), np.asarray(st, np.uint8), np.asarray(A, np.int64)

    def _swap(self, state, f, m_, l):
        if np.asarray(state["circ"])[f] == 1:
            return 0, 0, CIRCULAR, 0
        m, sx, sy = _members(state, f, m_, l)
        S = self.new_layout(state, f, m_, l)
        c_old = sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, state)[0]
        c_new = sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, S)[0]
        masks = []
        for g in (m[sx], m[sy], np.concatenate([m[:sx.start], m[sy.stop:]])):
            k = np.zeros(self.n, bool); k[g] = True
            masks.append(k[self.bin_of])
        total, absum, bad = 0, 0, False
        r, c = self.row, self.col
        sel = np.zeros(len(r), bool)
        for A_, B_ in self.groups(*masks):
            sel |= (A_[r] & B_[c]) | (B_[r] & A_[c])
        sd = np.abs(c_new[c] - c_new[r]).astype(np.float32)
        contacts = int(np.rint(self.count[sel & (sd < self.p[5])]).sum())
        rs, cs, ob = r[sel], c[sel], self.count[sel]
        old, new = self.cis(rs, cs, c_old), self.cis(rs, cs, c_new)
        with np.errstate(all="ignore"):
            v = ob * (np.log(new.astype(np.float64)) - np.log(old.astype(np.float64)))
        v = np.where(new == old, 0.0, v)
        bad |= not np.isfinite(v).all()
        t = np.rint(v[np.isfinite(v)] * Q).astype(np.int64)
        total += int(t.sum()); absum += int(np.abs(t).sum())
        subs = np.arange(len(self.bin_of))
        for A_, B_ in self.groups(*masks):                            # mass per fragment pair, A_'s fragment outer
            SA, SB = subs[A_], subs[B_]
            if len(SA) == 0 or len(SB) == 0:
                continue
            sa, sb = np.repeat(SA, len(SB)), np.tile(SB, len(SA))
            old, new = self.cis(sa, sb, c_old), self.cis(sa, sb, c_new)
            key = self.bin_of[sa] * self.n + self.bin_of[sb]
            u, inv = np.unique(key, return_inverse=True)
            acc = np.zeros(len(u))
            np.add.at(acc, inv, new.astype(np.float64) - old.astype(np.float64))   # (in sub-fragment order)
            bad |= not np.isfinite(acc).all()
            t = -np.rint(acc[np.isfinite(acc)] * Q).astype(np.int64)
            total += int(t.sum()); absum += int(np.abs(t).sum())
        return (0 if bad else total), contacts, (NONFINITE if bad else VALID), absum


def restatement(P, quirk=False, cls=Restatement):
    return cls(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
               P["param_simu"], P["coo_row"], P["coo_col"], P["coo_val"], quirk=quirk)


class Window(WR.Window):
    """swaps(state, first, mid, last): the same numbers, vectorised over the swaps of a call (their spans are disjoint: a bin has at
    most one swap and one role in it)."""

    def swaps(self, state, first, mid, last, parts=None):
        first, mid, last = (np.asarray(x, np.int64).reshape(-1) for x in (first, mid, last))
        nb = len(first)
        idc, pos, circ = (np.asarray(state[k], np.int64) for k in ("id_c", "pos", "circ"))
        start, ln = np.asarray(state["start_bp"], np.int64), np.asarray(state["len_bp"], np.int64)
        fwd = np.asarray(state["ori"]) == 1
        assert (idc[first] == idc[last]).all() and (idc[first] == idc[mid]).all() and (pos[first] <= pos[mid]).all() and (pos[mid] < pos[last]).all()
        members = {lab: m for lab, m in WR._runs(idc, pos)}
        status = np.full(nb, VALID, np.uint8)
        sw = np.full(self.n, -1, np.int64)
        role = np.zeros(self.n, np.int64)
        new_start = start.copy()
        for k in range(nb):
            if circ[first[k]] == 1:
                status[k] = CIRCULAR
                continue
            m = members[int(idc[first[k]])]
            X, Y = m[pos[first[k]]:pos[mid[k]] + 1], m[pos[mid[k]] + 1:pos[last[k]] + 1]
            assert (sw[X] == -1).all() and (sw[Y] == -1).all(), "spans overlap"
            sw[X] = k; sw[Y] = k; role[Y] = 1
            new_start[X] = start[X] + ln[Y].sum()
            new_start[Y] = start[Y] - ln[X].sum()
        allb = np.arange(self.n)
        C_old = self.centres(allb, start, fwd)
        C_new = self.centres(allb, new_start, fwd)
        q = np.zeros(nb, np.int64); A = np.zeros(nb, np.int64); cnt = np.zeros(nb, np.int64); bad = np.zeros(nb, bool)
        P_ = {k: np.zeros(nb, np.int64) for k in ("contacts", "mass")}

        def add(cls, k, t, b):
            np.add.at(q, k, t); np.add.at(A, k, np.abs(t)); np.logical_or.at(bad, k, b); np.add.at(P_[cls], k, t)
        # ---- contacts of one contig: X x Y of one swap once with both moved; sides of different swaps each with that side moved alone
        a, sa = self._sub(self.row)
        b, sb = self._sub(self.col)
        aa, ab = self.acc_s[a, sa], self.acc_s[b, sb]
        co_a, co_b, cn_a, cn_b = C_old[a, sa], C_old[b, sb], C_new[a, sa], C_new[b, sb]
        cis = idc[a] == idc[b]
        old_all = np.abs(co_b - co_a).astype(np.float32)
        for sel, key, ca, cb in ((cis & (sw[a] == sw[b]) & (sw[a] >= 0) & (role[a] != role[b]), sw[a], cn_a, cn_b),
                                 (cis & (sw[a] != sw[b]) & (sw[a] >= 0), sw[a], cn_a, co_b),
                                 (cis & (sw[a] != sw[b]) & (sw[b] >= 0), sw[b], co_a, cn_b)):
            k = np.nonzero(sel)[0]
            sd = np.abs(cb[k] - ca[k]).astype(np.float32)
            t, bd = self.contact_terms(self.count[k], self.cis(aa[k], ab[k], sd), self.cis(aa[k], ab[k], old_all[k]))
            add("contacts", key[k], t, bd)
            np.add.at(cnt, key[k], np.where(sd < self.d_max, np.rint(self.count[k]), 0).astype(np.int64))
        # ---- mass: a pair takes part when the smaller of its two gaps (before, after) is within reach
        XS, YS, KS, BOTH = [], [], [], []
        R = self.reach
        for k in np.nonzero(status == VALID)[0]:
            m = members[int(idc[first[k]])]
            p0, pm, p1 = int(pos[first[k]]), int(pos[mid[k]]), int(pos[last[k]])
            s0, sm, e1 = int(start[first[k]]), int(start[mid[k]] + ln[mid[k]]), int(start[last[k]] + ln[last[k]])
            X, Y, L, Rr = m[p0:pm + 1], m[pm + 1:p1 + 1], m[:p0], m[p1 + 1:]
            X = X[np.minimum(start[X] - s0, sm - (start[X] + ln[X])) <= R]
            Y = Y[np.minimum(start[Y] - sm, e1 - (start[Y] + ln[Y])) <= R]
            gL, gR = s0 - (start[L] + ln[L]), start[Rr] - e1
            L, gL, Rr, gR = L[gL <= R], gL[gL <= R], Rr[gR <= R], gR[gR <= R]
            dlX, drX = start[X] - s0, sm - (start[X] + ln[X])
            dlY, drY = start[Y] - sm, e1 - (start[Y] + ln[Y])
            for U, V, near, both in ((X, L, dlX[:, None] + gL[None, :] <= R, False), (X, Rr, drX[:, None] + gR[None, :] <= R, False),
                                     (Y, L, dlY[:, None] + gL[None, :] <= R, False), (Y, Rr, drY[:, None] + gR[None, :] <= R, False),
                                     (X, Y, np.minimum(drX[:, None] + dlY[None, :], dlX[:, None] + drY[None, :]) <= R, True)):
                i, j = np.nonzero(near)
                XS.append(U[i]); YS.append(V[j]); KS.append(np.full(len(i), k)); BOTH.append(np.full(len(i), both))
        if XS:
            X, Y, K, B = np.concatenate(XS), np.concatenate(YS), np.concatenate(KS), np.concatenate(BOTH)
            for i0 in range(0, len(X), WR.CHUNK):
                x, y, kk, bb = X[i0:i0 + WR.CHUNK], Y[i0:i0 + WR.CHUNK], K[i0:i0 + WR.CHUNK], B[i0:i0 + WR.CHUNK]
                cy_new = np.where(bb[:, None], C_new[y], C_old[y])      # (a flank fragment of another swap of the call stays put)
                t, bd = self.mass(x, y, ("cis", C_new[x], cy_new), ("cis", C_old[x], C_old[y]))
                add("mass", kk, t, bd)
        status[bad & (status == VALID)] = NONFINITE
        q[status != VALID] = 0
        if parts is not None:
            parts.update(P_)
        return q, cnt, status, A


def window(P, quirk=False, cls=Window):
    return cls(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
               P["param_simu"], P["coo_row"], P["coo_col"], P["coo_val"], quirk=quirk)


# the planted transpositions of the end-to-end tests: (chromosome, position, |X|, |Y|), X moved behind Y
PLANTS = ((0, 60, 1, 1), (0, 150, 2, 5), (0, 300, 3, 3), (1, 10, 6, 2), (1, 120, 1, 4), (2, 100, 20, 30), (3, 30, 2, 2))


def planted(s, plants=PLANTS):
    """(the layout with the plants applied, and the (first, mid, last) that name in it the swaps that undo them)."""
    chroms = list(LR.contigs_of(s).values())
    first = np.array([chroms[c][p] for c, p, x, y in plants])
    mid = np.array([chroms[c][p + x - 1] for c, p, x, y in plants])
    last = np.array([chroms[c][p + x + y - 1] for c, p, x, y in plants])
    return (swap_layout(s, first, mid, last),) + tuple(swapped_back(s, first, mid, last))


assert_true_chromosomes = FR.assert_true_chromosomes_and_orientations
