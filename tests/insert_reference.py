"""TEST INFRASTRUCTURE -- numpy restatement of graal_insertions (graal_amd/csrc/insert.h), by brute force: for every piece (a linear contig
of 1 .. max_piece_frags fragments), every junction f -> g of another linear contig T and both orientations, the inserted layout T1, P, T2 is
built field by field (tests/link_reference.py's layout) and every sub-fragment pair whose price can change is re-priced with the correctly
rounded float32 model of tests/junction_reference.py: P x T (trans now, cis after), T1 x T2 (cis at d, cis at d + len(P)), and -- with
the trans-branch indexing -- P against every fragment outside P u T (trans in both layouts; a reversed P flips its mixed bins).  Pairs
inside P, T1 and T2 count as unchanged.  A term is rounded to Q once (a contact; a fragment pair's mass).  Not product code.
"""
import numpy as np

from tests import link_reference as LR
from tests.link_reference import Q, contig_lists, contigs_of, layout  # noqa: F401  (Q: re-exported for the tests)
from tests.sim_reference import sub_records

VALID, NONFINITE = 0, 1


def pieces_of(state, max_piece_frags):
    """{label: fragments in position order} of the pieces: linear contigs of 1 .. max_piece_frags fragments."""
    circ = np.asarray(state["circ"])
    return {c: m for c, m in contigs_of(state).items() if circ[m[0]] == 0 and len(m) <= max_piece_frags}


def junctions_of(state):
    """{fragment f: label} of the target junctions: next[f] != -1 in a linear contig."""
    circ, nxt, idc = (np.asarray(state[k]) for k in ("circ", "next", "id_c"))
    return {int(f): int(idc[f]) for f in np.nonzero((circ == 0) & (nxt != -1))[0]}


def insert_layout(state, head, f, rev):
    """The inserted layout: the contig T of f cut between f and next[f], the piece whose position-0 fragment is `head` put in between
    (rev 0: its head next to f; rev 1: reversed, its tail next to f).  T keeps its label and direction; every other contig is untouched."""
    lists = contig_lists(state)
    idc = np.asarray(state["id_c"])
    cp, ct = int(idc[head]), int(idc[f])
    assert cp != ct
    P, T = lists[cp], lists[ct]
    assert P[0][0] == head
    if rev:
        P = [(x, -o) for x, o in reversed(P)]
    k = [x for x, _ in T].index(f) + 1
    assert k < len(T)
    labels = [c for c in sorted(lists) if c != cp]
    contigs = [T[:k] + P + T[k:] if c == ct else lists[c] for c in labels]
    circ = np.asarray(state["circ"])
    rings = {i for i, fr in enumerate(contigs) if circ[fr[0][0]] == 1}
    s = layout(state["len_bp"], contigs, rings)
    s["id_c"][:] = np.asarray(labels)[s["id_c"]]
    return s


class Restatement(LR.Restatement):
    """Static data of a problem; insertions(state, max_piece_frags) restates graal_insertions for layout `state`."""

    def insertions(self, state, max_piece_frags=1):
        """(piece, after, rev, q in Q, contacts, status, sum of |terms| in Q): int64 / uint8 arrays sorted by (after, piece, rev)."""
        pieces = pieces_of(state, max_piece_frags)
        juncs = junctions_of(state)
        idc = np.asarray(state["id_c"])
        lab_sub = idc[self.bin_of]
        centre_old, _, _, _ = sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, state)
        r, c = self.row, self.col
        out = []
        for cp, pm in pieces.items():
            inP = lab_sub == cp
            for f, ct in juncs.items():
                if ct == cp:
                    continue
                inT = lab_sub == ct
                pt = (inP[r] & inT[c]) | (inT[r] & inP[c])
                if not pt.any():
                    continue
                for rev in (0, 1):
                    x = self._insertion(state, int(pm[0]), f, rev, cp, ct, inP, inT, pt, lab_sub, centre_old)
                    if x is not None:
                        out.append(x)
        if not out:
            z = np.zeros(0, np.int64)
            return z, z, z, z, z, np.zeros(0, np.uint8), z
        out.sort(key=lambda t: (t[1], t[0], t[2]))
        p, a, rv, q, cn, st, ab = (np.array(x) for x in zip(*out))
        return p, a, rv, q, cn, st.astype(np.uint8), ab

    def _insertion(self, state, head, f, rev, cp, ct, inP, inT, pt, lab_sub, centre_old):
        S = insert_layout(state, head, f, rev)
        centre_new, _, _, _ = sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, S)
        d_max = self.p[5]
        r, c = self.row, self.col
        sd = np.abs(centre_new[c] - centre_new[r]).astype(np.float32)
        in_win = pt & (sd < d_max)
        if not in_win.any():
            return None                                                   # (not listed: no contact inside the window)
        contacts = int(np.rint(self.count[in_win]).sum())
        fwd = np.asarray(state["ori"]) == 1
        fwd_new = np.asarray(S["ori"]) == 1
        pos = np.asarray(state["pos"])
        t1_bins = np.asarray(state["id_c"]) == ct
        t1_bins &= pos <= pos[f]
        in1 = inT & t1_bins[self.bin_of]
        in2 = inT & ~t1_bins[self.bin_of]
        rest = ~(inP | inT)
        total, absum, bad = 0, 0, False
        # contacts: P x T (trans -> cis), T1 x T2 (cis -> cis), with the indexing P x rest (trans -> trans)
        t12 = (in1[r] & in2[c]) | (in2[r] & in1[c])
        pr = (inP[r] & rest[c]) | (rest[r] & inP[c]) if self.quirk else np.zeros_like(pt)
        sel = pt | t12 | pr
        rs, cs, ob = r[sel], c[sel], self.count[sel]
        kind = np.where(pt[sel], 0, np.where(t12[sel], 1, 2))
        old = np.where(kind == 1, self.cis(rs, cs, centre_old), self.trans(rs, cs, fwd))
        new = np.where(kind == 2, self.trans(rs, cs, fwd_new), self.cis(rs, cs, centre_new))
        with np.errstate(all="ignore"):
            v = ob * (np.log(new.astype(np.float64)) - np.log(old.astype(np.float64)))
        v = np.where(new == old, 0.0, v)
        if not np.isfinite(v).all():
            bad = True
        t = np.rint(v[np.isfinite(v)] * Q).astype(np.int64)
        total += int(t.sum()); absum += int(np.abs(t).sum())
        # mass: fragment pairs of P x T, T1 x T2 and (indexing) P x rest
        subs = np.arange(len(self.bin_of))
        SP, ST, S1, S2 = subs[inP], subs[inT], subs[in1], subs[in2]
        groups = [(SP, ST, 0), (S1, S2, 1)]
        if self.quirk:
            groups.append((SP, subs[rest], 2))
        for A, B, kind in groups:
            if len(A) == 0 or len(B) == 0:
                continue
            sa, sb = np.repeat(A, len(B)), np.tile(B, len(A))
            if kind == 1:
                old = self.cis(sa, sb, centre_old).astype(np.float64)
                new = self.cis(sa, sb, centre_new).astype(np.float64)
            else:
                old = self.trans(sa, sb, fwd).astype(np.float64)
                new = (self.cis(sa, sb, centre_new) if kind == 0 else self.trans(sa, sb, fwd_new)).astype(np.float64)
            key = self.bin_of[sa] * self.n + self.bin_of[sb]
            u, inv = np.unique(key, return_inverse=True)
            acc = np.zeros(len(u))
            np.add.at(acc, inv, new - old)
            if not np.isfinite(acc).all():
                bad = True
            t = -np.rint(acc[np.isfinite(acc)] * Q).astype(np.int64)
            total += int(t.sum()); absum += int(np.abs(t).sum())
        return head, f, rev, (0 if bad else total), contacts, (NONFINITE if bad else VALID), absum


def restatement(P, quirk=False):
    return Restatement(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
                       P["param_simu"], P["coo_row"], P["coo_col"], P["coo_val"], quirk=quirk)
