"""TEST INFRASTRUCTURE -- numpy restatements of graal_block_flips (graal_amd/csrc/flips.h).  flip_layout() writes the layout with blocks
reversed in place.  Restatement (brute force, in the style of tests/link_reference.py) builds that layout per block and re-prices every
sub-fragment pair whose price can change with the correctly rounded float32 model: block x rest of the contig (cis in both layouts) and,
with the trans-branch indexing, block x every other contig (trans in both).  Window (on tests/window_reference.py's pricing, mass,
contact-term and mirror helpers) gives the same numbers for problems of ~10^4 fragments by enumerating a fragment pair's mass only
where one of its two gaps is inside the window.  A term is rounded to Q once (a contact; a fragment pair's mass, the block's fragment
outer).  Per block: (q, contacts, status, A), A the sum of |terms| in Q.  No engine record, slot numbering or kernel output.  Not
product code.
"""
import numpy as np

from tests import link_reference as LR
from tests import window_reference as WR
from tests.sim_reference import sub_records

f32 = np.float32
Q = LR.Q
VALID, WHOLE, CIRCULAR, NONFINITE = 0, 1, 2, 3


def _members(state, f, l):
    """(the contig's fragments in position order, the block's slice of them)."""
    idc, pos = np.asarray(state["id_c"]), np.asarray(state["pos"])
    assert idc[f] == idc[l] and pos[f] <= pos[l]
    m = np.nonzero(idc == idc[f])[0]
    m = m[np.argsort(pos[m])]
    return m, slice(int(pos[f]), int(pos[l]) + 1)


def flip_layout(state, first, last):
    """The layout with every block (first[k] .. last[k]; scalars: one block) reversed in place: the block keeps its bp interval, a
    fragment at (s, l) goes to s0 + e1 - (s + l), ori changes sign, positions are mirrored inside the block, prev / next follow."""
    s = {k: np.array(v, dtype=np.int32, copy=True) for k, v in state.items()}
    first, last = np.atleast_1d(first), np.atleast_1d(last)
    touched = set()
    for f, l in zip(first, last):
        m, sl = _members(state, int(f), int(l))
        b = m[sl]
        assert not (touched & set(b.tolist())), "blocks overlap"
        touched |= set(b.tolist())
        s0 = int(state["start_bp"][b[0]]); e1 = int(state["start_bp"][b[-1]]) + int(state["len_bp"][b[-1]])
        s["start_bp"][b] = s0 + e1 - (np.asarray(state["start_bp"])[b] + np.asarray(state["len_bp"])[b])
        s["ori"][b] = -np.asarray(state["ori"])[b]
        s["pos"][b] = int(state["pos"][b[0]]) + int(state["pos"][b[-1]]) - np.asarray(state["pos"])[b]
    circ = np.asarray(s["circ"])
    for c, m in LR.contigs_of(s).items():                             # prev / next along the new position order
        ring = circ[m[0]] == 1 and len(m) > 1
        s["prev"][m] = np.concatenate([[m[-1] if ring else -1], m[:-1]])
        s["next"][m] = np.concatenate([m[1:], [m[0] if ring else -1]])
        if circ[m[0]] == 1 and len(m) == 1:
            s["prev"][m] = state["prev"][m]; s["next"][m] = state["next"][m]
    return s


def reverse_contig(state, label):
    """The layout with the whole contig `label` turned round (what graal_edit_layout's canonical chain order may do)."""
    m = LR.contigs_of(state)[label]
    return flip_layout(state, m[0], m[-1])


def same_layout(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("pos", "start_bp", "ori", "prev", "next", "l_cont", "l_cont_bp", "circ"))


def _status_only(state, f, l):
    m, sl = _members(state, f, l)
    if np.asarray(state["circ"])[f] == 1:
        return CIRCULAR
    if sl.start == 0 and sl.stop == len(m):
        return WHOLE
    return None


class Restatement(LR.Restatement):
    """flips(state, first, last) restates graal_block_flips by brute force, one block at a time."""

    def new_centres(self, flipped):
        return sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, flipped)[0]

    def flank(self, state, m, sl):
        """The fragments of the block's contig outside the block."""
        return np.concatenate([m[:sl.start], m[sl.stop:]])

    def flips(self, state, first, last):
        out = [self._flip(state, int(f), int(l)) for f, l in zip(first, last)]
        q, c, st, A = (np.array(x) for x in zip(*out)) if out else ([], [], [], [])
        return np.asarray(q, np.int64), np.asarray(c, np.int64), np.asarray(st, np.uint8), np.asarray(A, np.int64)

    def _flip(self, state, f, l):
        st = _status_only(state, f, l)
        if st is not None:
            return 0, 0, st, 0
        m, sl = _members(state, f, l)
        F = flip_layout(state, f, l)
        c_old = sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, state)[0]
        c_new = self.new_centres(F)
        fwd, fwd_new = np.asarray(state["ori"]) == 1, np.asarray(F["ori"]) == 1
        in_b = np.zeros(self.n, bool); in_b[m[sl]] = True
        in_r = np.zeros(self.n, bool); in_r[self.flank(state, m, sl)] = True
        in_o = np.asarray(state["id_c"]) != np.asarray(state["id_c"])[f]
        B, R_, O = in_b[self.bin_of], in_r[self.bin_of], in_o[self.bin_of]
        total, absum, bad = 0, 0, False
        # contacts: block x rest (cis -> cis); with the indexing, block x the other contigs (trans -> trans)
        r, c = self.row, self.col
        cis = (B[r] & R_[c]) | (R_[r] & B[c])
        sd = np.abs(c_new[c] - c_new[r]).astype(np.float32)
        contacts = int(np.rint(self.count[cis & (sd < self.p[5])]).sum())
        sel = cis | (((B[r] & O[c]) | (O[r] & B[c])) if self.quirk else np.zeros_like(cis))
        rs, cs, ob = r[sel], c[sel], self.count[sel]
        old = np.where(cis[sel], self.cis(rs, cs, c_old), self.trans(rs, cs, fwd))
        new = np.where(cis[sel], self.cis(rs, cs, c_new), self.trans(rs, cs, fwd_new))
        with np.errstate(all="ignore"):
            v = ob * (np.log(new.astype(np.float64)) - np.log(old.astype(np.float64)))
        v = np.where(new == old, 0.0, v)
        bad |= not np.isfinite(v).all()
        t = np.rint(v[np.isfinite(v)] * Q).astype(np.int64)
        total += int(t.sum()); absum += int(np.abs(t).sum())
        # mass: fragment pairs of block x rest, and (indexing) of block x the other contigs; the block's fragment outer
        subs = np.arange(len(self.bin_of))
        SB = subs[B]
        for S2, is_cis in ((subs[R_], True), (subs[O], False)):
            if len(S2) == 0 or len(SB) == 0 or not (is_cis or self.quirk):
                continue
            sa, sb = np.repeat(SB, len(S2)), np.tile(S2, len(SB))
            if is_cis:
                old, new = self.cis(sa, sb, c_old), self.cis(sa, sb, c_new)
            else:
                old, new = self.trans(sa, sb, fwd), self.trans(sa, sb, fwd_new)
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
    """flips(state, first, last): the same numbers, vectorised over the blocks of a call (they are disjoint: a bin has one block)."""

    one_flank = False      # (a flaw for the tests: the mass of the left flank only)

    def flips(self, state, first, last, parts=None):
        first, last = np.asarray(first, np.int64), np.asarray(last, np.int64)
        nb = len(first)
        idc, pos, circ = (np.asarray(state[k], np.int64) for k in ("id_c", "pos", "circ"))
        start, ln = np.asarray(state["start_bp"], np.int64), np.asarray(state["len_bp"], np.int64)
        fwd = np.asarray(state["ori"]) == 1
        assert (idc[first] == idc[last]).all() and (pos[first] <= pos[last]).all()
        members = {lab: m for lab, m in WR._runs(idc, pos)}
        status = np.full(nb, VALID, np.uint8)
        blk = np.full(self.n, -1, np.int64)
        new_start = start.copy()
        for k in range(nb):
            m = members[int(idc[first[k]])]
            if circ[first[k]] == 1:
                status[k] = CIRCULAR
            elif pos[first[k]] == 0 and pos[last[k]] == len(m) - 1:
                status[k] = WHOLE
            else:
                b = m[pos[first[k]]:pos[last[k]] + 1]
                assert (blk[b] == -1).all(), "blocks overlap"
                blk[b] = k
                new_start[b] = start[first[k]] + start[last[k]] + ln[last[k]] - (start[b] + ln[b])
        fwd_new = np.where(blk >= 0, ~fwd, fwd)
        C_old = self.centres(np.arange(self.n), start, fwd)
        C_new = self.centres(np.arange(self.n), new_start, fwd_new)
        q = np.zeros(nb, np.int64); A = np.zeros(nb, np.int64); cnt = np.zeros(nb, np.int64); bad = np.zeros(nb, bool)
        P_ = {k: np.zeros(nb, np.int64) for k in ("contacts", "mass", "mirror_contacts", "mirror")}

        def add(cls, k, t, b):
            np.add.at(q, k, t); np.add.at(A, k, np.abs(t)); np.logical_or.at(bad, k, b); np.add.at(P_[cls], k, t)
        # ---- contacts of one contig whose sides have different blocks: each side's block is priced with only that block flipped
        a, sa = self._sub(self.row)
        b, sb = self._sub(self.col)
        aa, ab = self.acc_s[a, sa], self.acc_s[b, sb]
        same = (idc[a] == idc[b]) & (blk[a] != blk[b])
        co_a, co_b = C_old[a, sa], C_old[b, sb]
        for side, other_c in ((a, co_b), (b, co_a)):
            k = np.nonzero(same & (blk[side] >= 0))[0]
            mine_new = (C_new[a, sa] if side is a else C_new[b, sb])[k]
            sd = np.abs(other_c[k] - mine_new).astype(np.float32)
            new = self.cis(aa[k], ab[k], sd)
            old = self.cis(aa[k], ab[k], np.abs(co_b[k] - co_a[k]).astype(np.float32))
            t, bd = self.contact_terms(self.count[k], new, old)
            add("contacts", blk[side][k], t, bd)
            np.add.at(cnt, blk[side][k], np.where(sd < self.d_max, np.rint(self.count[k]), 0).astype(np.int64))
        if self.quirk:                                                 # the lower-id bin's orientation picks the trans price's indexing
            lo_is_a = a < b
            lo = np.where(lo_is_a, a, b)
            k = np.nonzero((idc[a] != idc[b]) & (blk[lo] >= 0) & self.mixed[lo])[0]
            new = self.trans(a[k], b[k], aa[k], ab[k], fwd_new[a[k]], fwd_new[b[k]])
            old = self.trans(a[k], b[k], aa[k], ab[k], fwd[a[k]], fwd[b[k]])
            t, bd = self.contact_terms(self.count[k], new, old)
            add("mirror_contacts", blk[lo[k]], t, bd)
        # ---- mass: the block's fragments within reach of a boundary x the flank fragments within reach of it
        XS, YS, KS = [], [], []
        for k in np.nonzero(status == VALID)[0]:
            m = members[int(idc[first[k]])]
            p0, p1 = int(pos[first[k]]), int(pos[last[k]])
            s0, e1 = int(start[first[k]]), int(start[last[k]] + ln[last[k]])
            B = m[p0:p1 + 1]
            dm = np.minimum(start[B] - s0, e1 - (start[B] + ln[B]))
            B, dm = B[dm <= self.reach], dm[dm <= self.reach]
            L, R_ = m[:p0], (m[p1 + 1:] if not self.one_flank else m[:0])
            Y = np.concatenate([L, R_])
            g = np.concatenate([s0 - (start[L] + ln[L]), start[R_] - e1])
            Y, g = Y[g <= self.reach], g[g <= self.reach]
            i, j = np.nonzero(dm[:, None] + g[None, :] <= self.reach)
            XS.append(B[i]); YS.append(Y[j]); KS.append(np.full(len(i), k))
            if self.quirk:
                t_, a_, b_ = self._mirror(m[p0:p1 + 1], ~fwd[m[p0:p1 + 1]], fwd[m[p0:p1 + 1]], m)
                q[k] += t_; A[k] += a_; bad[k] |= b_; P_["mirror"][k] += t_
        if XS:
            X, Y, K = np.concatenate(XS), np.concatenate(YS), np.concatenate(KS)
            for i0 in range(0, len(X), WR.CHUNK):
                x, y, kk = X[i0:i0 + WR.CHUNK], Y[i0:i0 + WR.CHUNK], K[i0:i0 + WR.CHUNK]
                t, bd = self.mass(x, y, ("cis", C_new[x], C_old[y]), ("cis", C_old[x], C_old[y]))
                add("mass", kk, t, bd)
        status[bad & (status == VALID)] = NONFINITE
        q[status != VALID] = 0
        if parts is not None:
            parts.update(P_)
        return q, cnt, status, A


def window(P, quirk=False, cls=Window):
    return cls(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
               P["param_simu"], P["coo_row"], P["coo_col"], P["coo_val"], quirk=quirk)


# the planted inversions of the end-to-end test: (chromosome, position, fragments)
PLANTS = ((0, 50, 2), (0, 120, 5), (0, 250, 40), (1, 0, 7), (1, 100, 150), (2, 170, 30), (3, 40, 3))


def planted(s):
    chroms = list(LR.contigs_of(s).values())
    first = np.array([chroms[c][p] for c, p, _ in PLANTS])
    last = np.array([chroms[c][p + w - 1] for c, p, w in PLANTS])
    return flip_layout(s, first, last), first, last


def assert_true_chromosomes_and_orientations(got, s):
    """Every chromosome of the truth `s` is one contig of `got` in its true order with every fragment's true ori, or wholly reversed."""
    truth = LR.contigs_of(s)
    assert len(np.unique(got["id_c"])) == len(truth)
    for c, m in truth.items():
        assert len(np.unique(got["id_c"][m])) == 1
        order = m[np.argsort(got["pos"][m])]
        same = np.array_equal(order, m) and np.array_equal(got["ori"][m], np.asarray(s["ori"])[m])
        turned = np.array_equal(order, m[::-1]) and np.array_equal(got["ori"][m], -np.asarray(s["ori"])[m])
        assert same or turned, c
