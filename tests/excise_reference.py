"""TEST INFRASTRUCTURE -- numpy restatements of graal_block_excisions (graal_amd/csrc/excise.h).  excise_layout() writes the layout with
runs X of fragments cut out of their contigs, the gap closed behind each and every X a linear contig of its own, field by field, in the
contig's own direction (no chain reversal).  Restatement (brute force, in the style of tests/swap_reference.py) builds that layout per
span and re-prices every sub-fragment pair whose price can change with the correctly rounded float32 model: X x (L u R) from cis to
trans (the trans-branch indexing when `quirk`; nothing is turned round, so the trans prices against other contigs stay), L x R from cis
to cis with R moved len_bp(X) down.  Window (on tests/window_reference.py's pricing, mass and contact-term helpers) gives the same
numbers for problems of ~10^4 fragments: a fragment pair's mass only where its gap (X x rest: now; L x R: after the excision) is inside
the window, plus the far pairs of X x rest that the indexing prices apart.  A term is rounded to Q once (a contact; a fragment pair's
mass, X's fragment outer for X x rest, L's for L x R).  Per span: (q, contacts, status, A), A the sum of |terms| in Q; contacts = the
summed count of the X x (L u R) contacts whose CURRENT centre distance is below d_max.  No engine record, slot numbering or kernel
output.  Not product code.
"""
import numpy as np

from tests import flip_reference as FR
from tests import link_reference as LR
from tests import window_reference as WR
from tests.sim_reference import sub_records

f32 = np.float32
Q = LR.Q
VALID, WHOLE, CIRCULAR, NONFINITE = 0, 1, 2, 3

_members = FR._members
_status_only = FR._status_only


def excise_layout(state, first, last):
    """The layout with, for every span (scalars: one span), the run X = first .. last cut out: the fragments behind it in its contig get
    start_bp - len_bp(X) and pos - |X|, X becomes a linear contig of its own under a fresh label (the layout's highest + 1 + the span's
    index in the call), start_bp counted from 0, ori kept; l_cont, l_cont_bp, prev and next follow.  A span that is its whole contig
    changes nothing."""
    s = {k: np.array(v, dtype=np.int32, copy=True) for k, v in state.items()}
    start, ln, pos, idc = (np.asarray(state[k]).astype(np.int64) for k in ("start_bp", "len_bp", "pos", "id_c"))
    assert not np.asarray(state["circ"])[np.atleast_1d(first)].any(), "a span in a ring"
    fresh = int(idc.max()) + 1
    spans = [_members(state, int(f), int(l)) for f, l in zip(np.atleast_1d(first), np.atleast_1d(last))]
    cut = np.zeros(len(idc), bool)
    for m, sl in spans:
        assert not cut[m[sl]].any(), "spans overlap"
        cut[m[sl]] = len(m[sl]) < len(m)
    for k, (m, sl) in enumerate(spans):
        X = m[sl]
        if len(X) == len(m):
            continue
        R_ = m[sl.stop:][~cut[m[sl.stop:]]]                             # (several spans of a contig: each takes its own share off)
        s["start_bp"][R_] -= int(ln[X].sum()); s["pos"][R_] -= len(X)
        s["start_bp"][X] = start[X] - start[X[0]]; s["pos"][X] = pos[X] - pos[X[0]]
        s["id_c"][X] = fresh + k
    for c, m in LR.contigs_of(s).items():
        if np.asarray(s["circ"])[m[0]] == 1:
            continue
        s["l_cont"][m] = len(m); s["l_cont_bp"][m] = int(np.asarray(s["len_bp"])[m].astype(np.int64).sum())
        s["prev"][m] = np.concatenate([[-1], m[:-1]])
        s["next"][m] = np.concatenate([m[1:], [-1]])
    return s


def chains(state):
    """The layout as a set of contigs, each the tuple of its (fragment, ori) in position order or that of its reversal, whichever is
    smaller, with its circ flag: what two layouts share when they are equal up to labels and the reversal of whole contigs."""
    out = set()
    circ = np.asarray(state["circ"])
    for c, frags in LR.contig_lists(state).items():
        fwd = tuple(frags)
        rev = tuple((f, -o) for f, o in reversed(frags))
        out.add((min(fwd, rev), int(circ[frags[0][0]])))
    return out


class Restatement(LR.Restatement):
    """excisions(state, first, last) restates graal_block_excisions by brute force, one span at a time."""

    def excisions(self, state, first, last):
        out = [self._excise(state, int(f), int(l)) for f, l in zip(first, last)]
        q, c, st, A = (np.array(x) for x in zip(*out)) if out else ([], [], [], [])
        return np.asarray(q, np.int64), np.asarray(c, np.int64), np.asarray(st, np.uint8), np.asarray(A, np.int64)

    def _excise(self, state, f, l):
        st = _status_only(state, f, l)
        if st is not None:
            return 0, 0, st, 0
        m, sl = _members(state, f, l)
        S = excise_layout(state, f, l)
        c_old = sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, state)[0]
        c_new = sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, S)[0]
        fwd = np.asarray(state["ori"]) == 1
        masks = []
        for g in (m[sl], m[:sl.start], m[sl.stop:]):
            k = np.zeros(self.n, bool); k[g] = True
            masks.append(k[self.bin_of])
        X, L, R_ = masks
        rest = L | R_
        r, c = self.row, self.col
        xr = (X[r] & rest[c]) | (rest[r] & X[c])
        lr = (L[r] & R_[c]) | (R_[r] & L[c])
        sd_old = np.abs(c_old[c] - c_old[r]).astype(np.float32)
        contacts = int(np.rint(self.count[xr & (sd_old < self.p[5])]).sum())
        total, absum, bad = 0, 0, False
        sel = xr | lr
        rs, cs, ob = r[sel], c[sel], self.count[sel]
        old = self.cis(rs, cs, c_old)
        new = np.where(xr[sel], self.trans(rs, cs, fwd), self.cis(rs, cs, c_new))
        with np.errstate(all="ignore"):
            v = ob * (np.log(new.astype(np.float64)) - np.log(old.astype(np.float64)))
        v = np.where(new == old, 0.0, v)
        bad |= not np.isfinite(v).all()
        t = np.rint(v[np.isfinite(v)] * Q).astype(np.int64)
        total += int(t.sum()); absum += int(np.abs(t).sum())
        subs = np.arange(len(self.bin_of))
        for A_, B_, to_trans in ((X, rest, True), (L, R_, False)):      # mass per fragment pair, A_'s fragment outer
            SA, SB = subs[A_], subs[B_]
            if len(SA) == 0 or len(SB) == 0:
                continue
            sa, sb = np.repeat(SA, len(SB)), np.tile(SB, len(SA))
            old = self.cis(sa, sb, c_old)
            new = self.trans(sa, sb, fwd) if to_trans else self.cis(sa, sb, c_new)
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
    """excisions(state, first, last): the same numbers, vectorised over the spans of a call (they are disjoint: a bin has at most one
    span; a span is scored alone, the other spans of the call are part of its L and R, unmoved)."""

    def excisions(self, state, first, last, parts=None):
        first, last = np.asarray(first, np.int64).reshape(-1), np.asarray(last, np.int64).reshape(-1)
        nb = len(first)
        idc, pos, circ = (np.asarray(state[k], np.int64) for k in ("id_c", "pos", "circ"))
        start, ln = np.asarray(state["start_bp"], np.int64), np.asarray(state["len_bp"], np.int64)
        fwd = np.asarray(state["ori"]) == 1
        assert (idc[first] == idc[last]).all() and (pos[first] <= pos[last]).all()
        members = {lab: m for lab, m in WR._runs(idc, pos)}
        status = np.full(nb, VALID, np.uint8)
        sp = np.full(self.n, -1, np.int64)
        for k in range(nb):
            m = members[int(idc[first[k]])]
            if circ[first[k]] == 1:
                status[k] = CIRCULAR
            elif pos[first[k]] == 0 and pos[last[k]] == len(m) - 1:
                status[k] = WHOLE
            else:
                X = m[pos[first[k]]:pos[last[k]] + 1]
                assert (sp[X] == -1).all(), "spans overlap"
                sp[X] = k
        allb = np.arange(self.n)
        C_old = self.centres(allb, start, fwd)
        q = np.zeros(nb, np.int64); A = np.zeros(nb, np.int64); cnt = np.zeros(nb, np.int64); bad = np.zeros(nb, bool)
        P_ = {k: np.zeros(nb, np.int64) for k in ("contacts", "closing_contacts", "mass", "closing_mass", "far")}
        fed = np.zeros(nb, np.int64)                                   # L x R contacts with a non-zero term, per span (for the tests)
        closing = np.zeros(nb, np.int64)                               # of them, those at >= d_max now: the excision brings them inside

        def add(cls, k, t, b):
            np.add.at(q, k, t); np.add.at(A, k, np.abs(t)); np.logical_or.at(bad, k, b); np.add.at(P_[cls], k, t)
        # ---- X x rest contacts: a contact of one contig whose sides differ in span feeds each side's span, cis -> trans
        a, sa = self._sub(self.row)
        b, sb = self._sub(self.col)
        aa, ab = self.acc_s[a, sa], self.acc_s[b, sb]
        co_a, co_b = C_old[a, sa], C_old[b, sb]
        same = (idc[a] == idc[b]) & (a != b)
        sd_old = np.abs(co_b - co_a).astype(np.float32)
        k = np.nonzero(same & (sp[a] != sp[b]))[0]
        old = self.cis(aa[k], ab[k], sd_old[k])
        new = self.trans(a[k], b[k], aa[k], ab[k], fwd[a[k]], fwd[b[k]])
        t, bd = self.contact_terms(self.count[k], new, old)
        inw = np.where(sd_old[k] < self.d_max, np.rint(self.count[k]), 0).astype(np.int64)
        for side in (a, b):
            own = sp[side[k]] >= 0
            add("contacts", sp[side[k]][own], t[own], bd[own])
            np.add.at(cnt, sp[side[k]][own], inw[own])
        # ---- per span: L x R contacts, X x rest mass inside the window and the indexing's far pairs, L x R mass
        XS, YS, KS, KIND, LX = [], [], [], [], []
        R = self.reach
        rm = (~fwd) & self.mixed
        ks = np.nonzero(same)[0]
        ks = ks[np.argsort(idc[a[ks]], kind="stable")]
        labs, at = np.unique(idc[a[ks]], return_index=True)
        by_contig = {int(c): v for c, v in zip(labs, np.split(ks, at[1:]))}
        for k in np.nonzero(status == VALID)[0]:
            lab = int(idc[first[k]])
            m = members[lab]
            p0, p1 = int(pos[first[k]]), int(pos[last[k]])
            s0, e1 = int(start[first[k]]), int(start[last[k]] + ln[last[k]])
            lx = e1 - s0
            X, L, Rr = m[p0:p1 + 1], m[:p0], m[p1 + 1:]
            # L x R contacts: the partner in R at start_bp - lx
            kc = by_contig.get(lab, np.zeros(0, np.int64))
            pa, pb = pos[a[kc]], pos[b[kc]]
            kc = kc[((pa < p0) & (pb > p1)) | ((pb < p0) & (pa > p1))]
            if len(kc):
                hi_is_b = pos[b[kc]] > p1
                hb = np.where(hi_is_b, b[kc], a[kc]); hs = np.where(hi_is_b, sb[kc], sa[kc])
                c_lo = np.where(hi_is_b, co_a[kc], co_b[kc])
                c_hi = self.centres(hb, start[hb] - lx, fwd[hb])[np.arange(len(hb)), hs]
                new = self.cis(aa[kc], ab[kc], np.abs(c_hi - c_lo).astype(np.float32))
                t, bd = self.contact_terms(self.count[kc], new, self.cis(aa[kc], ab[kc], sd_old[kc]))
                add("closing_contacts", np.full(len(kc), k), t, bd)
                fed[k] += int(((t != 0) | bd).sum())
                closing[k] += int((((t != 0) | bd) & (sd_old[kc] >= self.d_max)).sum())
            dl, dr = start[X] - s0, e1 - (start[X] + ln[X])
            gL, gR = s0 - (start[L] + ln[L]), start[Rr] - e1
            for Y, near in ((L, dl[:, None] + gL[None, :] <= R), (Rr, dr[:, None] + gR[None, :] <= R)):
                i, j = np.nonzero(near)
                XS.append(X[i]); YS.append(Y[j]); KS.append(np.full(len(i), k)); KIND.append(np.zeros(len(i), np.int8)); LX.append(np.zeros(len(i), np.int64))
                if self.quirk and (rm[X].any() or rm[Y].any()) and len(Y):
                    fi, fj = self._far_quirk(X, Y, near, fwd)
                    XS.append(X[fi]); YS.append(Y[fj]); KS.append(np.full(len(fi), k)); KIND.append(np.full(len(fi), 2, np.int8)); LX.append(np.zeros(len(fi), np.int64))
            wl, wr = np.nonzero(gL <= R)[0], np.nonzero(gR <= R)[0]
            i, j = np.nonzero(gL[wl][:, None] + gR[wr][None, :] <= R)
            XS.append(L[wl[i]]); YS.append(Rr[wr[j]]); KS.append(np.full(len(i), k)); KIND.append(np.ones(len(i), np.int8)); LX.append(np.full(len(i), lx))
        if XS:
            X, Y, K, KD, LXS = (np.concatenate(v) for v in (XS, YS, KS, KIND, LX))
            for i0 in range(0, len(X), WR.CHUNK):
                x, y, kk, kd, lxs = (v[i0:i0 + WR.CHUNK] for v in (X, Y, K, KD, LXS))
                for kind, cls in ((0, "mass"), (2, "far"), (1, "closing_mass")):
                    s_ = kd == kind
                    if not s_.any():
                        continue
                    xs, ys = x[s_], y[s_]
                    if kind == 1:
                        new = ("cis", C_old[xs], self.centres(ys, start[ys] - lxs[s_], fwd[ys]))
                    else:
                        new = ("trans", fwd[xs], fwd[ys])
                    t, bd = self.mass(xs, ys, new, ("cis", C_old[xs], C_old[ys]))
                    add(cls, kk[s_], t, bd)
        status[bad & (status == VALID)] = NONFINITE
        q[status != VALID] = 0
        if parts is not None:
            parts.update(P_)
            parts["closing_fed"] = fed
            parts["closing_from_outside"] = closing
        return q, cnt, status, A


def window(P, quirk=False, cls=Window):
    return cls(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
               P["param_simu"], P["coo_row"], P["coo_col"], P["coo_val"], quirk=quirk)


# the misplaced runs of the end-to-end test: (chromosome, position, fragments, the chromosome and the position it is put in front of).
# Four sit in another chromosome, two more than two windows (~45 fragments) from home in their own; every home lies more than a window
# from its chromosome's ends, so that no end link competes with the insertion.
PLANTS = ((0, 60, 1, 1, 150), (0, 150, 2, 2, 80), (1, 40, 3, 0, 300), (2, 120, 1, 3, 50), (3, 40, 2, 3, 90), (0, 250, 3, 0, 30))


def planted(s, plants=PLANTS):
    """(the layout with the runs moved, first and last fragment of every run).  Positions are those of the true layout `s`."""
    orig = list(LR.contig_lists(s).values())
    runs = [orig[c][p:p + w] for c, p, w, _, _ in plants]
    gone = {f for r in runs for f, _ in r}
    out = []
    for ci, ch in enumerate(orig):
        new = []
        for i, (f, o) in enumerate(ch):
            for (_, _, _, dc, dp), r in zip(plants, runs):
                if dc == ci and dp == i:
                    new += r
            if f not in gone:
                new.append((f, o))
        out.append(new)
    return LR.layout(s["len_bp"], out), np.array([r[0][0] for r in runs]), np.array([r[-1][0] for r in runs])
