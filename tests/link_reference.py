"""TEST INFRASTRUCTURE -- numpy restatement of graal_end_links (graal_amd/csrc/links.h), by brute force: for every pair of ends of two
different linear contigs the canonical joined layout is built, and every sub-fragment pair whose price can change is re-priced with the
correctly rounded float32 model of tests/junction_reference.py -- the pairs of A x B (trans now, cis after the join) and the pairs of
A u B against every other fragment (trans in both layouts; the trans-branch indexing may re-price them when A or B is reversed).  Pairs
inside A and inside B count as unchanged.  A term is rounded to Q once (a contact; a fragment pair's mass).  Not product code.
"""
import numpy as np

from tests.junction_reference import Q, rippe_cr  # noqa: F401  (Q: re-exported for the tests)
from tests.sim_reference import sub_records

f32 = np.float32
VALID, NONFINITE = 0, 1
FIELDS = ("pos", "id_c", "start_bp", "len_bp", "circ", "id", "prev", "next", "l_cont", "l_cont_bp", "ori", "rep", "activ", "id_d")


def rippe_vec(s, p):
    """rippe_cr over an array: float64 per operation, rounded to float32 after each one."""
    kuhn, lm, c1, slope, d, d_max, fact, v = [f32(x) for x in p]
    s = np.asarray(s, dtype=np.float32)
    n = (s * lm).astype(np.float32)
    if kuhn != f32(1):
        n = (n / kuhn).astype(np.float32)
    inner = ((n * n).astype(np.float32) + d).astype(np.float32)
    e = np.exp(((d - f32(2)) / inner).astype(np.float32).astype(np.float64)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        pw = np.power(s.astype(np.float64), np.float64(slope)).astype(np.float32)
    r = ((((c1 * pw).astype(np.float32) * e).astype(np.float32)) * fact).astype(np.float32)
    r = np.where((s > 0) & (s < d_max), r, f32(0)).astype(np.float32)
    return np.maximum(r, v).astype(np.float32)


def contigs_of(state):
    """{label: fragments in position order} of the layout."""
    idc, pos = np.asarray(state["id_c"]), np.asarray(state["pos"])
    out = {}
    for c in np.unique(idc):
        m = np.nonzero(idc == c)[0]
        out[int(c)] = m[np.argsort(pos[m])]
    return out


def ends_of(state, min_frags=1):
    """{end: label} of the eligible contigs (linear, >= min_frags fragments): end = 2 * fragment + side (0 head, 1 tail)."""
    circ = np.asarray(state["circ"])
    out = {}
    for c, m in contigs_of(state).items():
        if circ[m[0]] == 1 or len(m) < min_frags:
            continue
        out[2 * int(m[0])] = c
        out[2 * int(m[-1]) + 1] = c
    return out


def layout(lens, contigs, circular=()):
    """Fragment fields of a layout given as lists of (fragment, orientation) per contig (label = list index); `circular`: labels of rings."""
    n = len(lens)
    s = {k: np.zeros(n, np.int32) for k in FIELDS}
    s["len_bp"][:] = lens; s["id"][:] = np.arange(n); s["id_d"][:] = np.arange(n); s["activ"][:] = 1
    for c, frags in enumerate(contigs):
        run = 0
        tot = int(sum(int(lens[f]) for f, _ in frags))
        for p, (f, o) in enumerate(frags):
            s["pos"][f] = p; s["id_c"][f] = c; s["start_bp"][f] = run; s["ori"][f] = o
            s["prev"][f] = frags[p - 1][0] if p > 0 else -1
            s["next"][f] = frags[p + 1][0] if p + 1 < len(frags) else -1
            s["l_cont"][f] = len(frags); s["l_cont_bp"][f] = tot
            s["circ"][f] = 1 if c in circular else 0
            run += int(lens[f])
    return s


def contig_lists(state):
    ori = np.asarray(state["ori"])
    return {c: [(int(f), int(ori[f])) for f in m] for c, m in contigs_of(state).items()}


def join_layout(state, ea, eb):
    """The canonical joined layout of ends ea < eb (different linear contigs): A oriented so that ea is its tail, B after it so that eb
    is its head, as m_paste writes it (the joined contig keeps A's label)."""
    assert ea < eb
    lists = contig_lists(state)
    idc = np.asarray(state["id_c"])
    ca, cb = int(idc[ea >> 1]), int(idc[eb >> 1])
    assert ca != cb
    A, B = lists[ca], lists[cb]
    if ea & 1 == 0:
        A = [(f, -o) for f, o in reversed(A)]
    if eb & 1 == 1:
        B = [(f, -o) for f, o in reversed(B)]
    assert A[-1][0] == ea >> 1 and B[0][0] == eb >> 1
    labels = sorted(lists)
    contigs = []
    for c in labels:
        if c == cb:
            continue
        contigs.append(A + B if c == ca else lists[c])
    circ = np.asarray(state["circ"])
    rings = {i for i, fr in enumerate(contigs) if circ[fr[0][0]] == 1}
    s = layout(state["len_bp"], contigs, rings)
    s["id_c"][:] = np.asarray([c for c in labels if c != cb])[s["id_c"]]   # (the labels as they were)
    return s


class Restatement:
    """Static data of a problem; links(state) restates graal_end_links for layout `state`."""

    def __init__(self, sub_id, sub_len_kb, sub_accu, nfpb, param, row, col, count, quirk=False):
        self.sub_id, self.sub_len_kb, self.sub_accu = sub_id, sub_len_kb, sub_accu
        sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
        self.n = len(sid)
        self.nsub = sid[:, 3]
        S = int(self.nsub.sum())
        self.bin_of = np.zeros(S, np.int64)
        for b in range(self.n):
            self.bin_of[sid[b, :self.nsub[b]]] = b
        acc = np.asarray(sub_accu, dtype=np.int64).reshape(-1, 3)
        self.acc = np.zeros(S, np.int64)
        for b in range(self.n):
            self.acc[sid[b, :self.nsub[b]]] = acc[b, :self.nsub[b]]
        self.last = np.array([acc[b, self.nsub[b] - 1] for b in range(self.n)], np.int64)
        self.mixed = np.array([len(set(acc[b, :self.nsub[b]].tolist())) > 1 for b in range(self.n)])
        self.nfpb = f32(nfpb)
        self.p = [f32(x) for x in param]
        self.row, self.col = np.asarray(row, np.int64), np.asarray(col, np.int64)
        self.count = np.asarray(count, dtype=np.float64)
        self.quirk = quirk

    def trans(self, sa, sb, fwd):
        ba, bb = self.bin_of[sa], self.bin_of[sb]
        aa, ab = self.acc[sa], self.acc[sb]
        if self.quirk:
            low = ba < bb
            aa = np.where(low & ~fwd[ba], self.last[ba], aa)
            ab = np.where(~low & ~fwd[bb], self.last[bb], ab)
        return (self.p[7] * ((aa * ab).astype(np.float32) / self.nfpb).astype(np.float32)).astype(np.float32)

    def cis(self, sa, sb, centre):
        norm = ((self.acc[sa] * self.acc[sb]).astype(np.float32) / self.nfpb).astype(np.float32)
        return (rippe_vec(np.abs(centre[sb] - centre[sa]).astype(np.float32), self.p) * norm).astype(np.float32)

    def links(self, state, min_frags=1):
        """(end_a int64[m], end_b int64[m], q int64[m] in Q, contacts int64[m], status uint8[m], sum of |terms| int64[m] in Q), sorted."""
        ends = ends_of(state, min_frags)
        fwd = np.asarray(state["ori"]) == 1
        idc = np.asarray(state["id_c"])
        lab_sub = idc[self.bin_of]
        d_max = self.p[5]
        out = []
        E = sorted(ends)
        for i, ea in enumerate(E):
            for eb in E[i + 1:]:
                ca, cb = ends[ea], ends[eb]
                if ca == cb:
                    continue
                r = self._link(state, ea, eb, ca, cb, fwd, lab_sub, d_max)
                if r is not None:
                    out.append(r)
        if not out:
            z = np.zeros(0, np.int64)
            return z, z, z, z, np.zeros(0, np.uint8), z
        a, b, q, c, st, ab = (np.array(x) for x in zip(*out))
        return a, b, q, c, st.astype(np.uint8), ab

    def _link(self, state, ea, eb, ca, cb, fwd, lab_sub, d_max):
        J = join_layout(state, ea, eb)
        centre_new, _, _, _ = sub_records(self.sub_id, self.sub_len_kb, self.sub_accu, J)
        fwd_new = np.asarray(J["ori"]) == 1
        inA, inB = lab_sub == ca, lab_sub == cb
        # contacts: A x B (trans -> cis) and A u B x rest (trans -> trans)
        r, c = self.row, self.col
        ab = (inA[r] & inB[c]) | (inB[r] & inA[c])
        out_ = (inA[r] | inB[r]) != (inA[c] | inB[c])
        if not ab.any():
            return None
        sd = np.abs(centre_new[c] - centre_new[r]).astype(np.float32)
        in_win = ab & (sd < d_max)
        if not in_win.any():
            return None                                                   # (not listed: no contact inside the window)
        contacts = int(np.rint(self.count[in_win]).sum())
        total, absum, bad = 0, 0, False
        sel = ab | (out_ if self.quirk else np.zeros_like(ab))
        rs, cs, ob = r[sel], c[sel], self.count[sel]
        old = self.trans(rs, cs, fwd)
        new = np.where(ab[sel], self.cis(rs, cs, centre_new), self.trans(rs, cs, fwd_new))
        with np.errstate(all="ignore"):
            v = ob * (np.log(new.astype(np.float64)) - np.log(old.astype(np.float64)))
        v = np.where(new == old, 0.0, v)
        if not np.isfinite(v).all():
            bad = True
        t = np.rint(v[np.isfinite(v)] * Q).astype(np.int64)
        total += int(t.sum()); absum += int(np.abs(t).sum())
        # mass: fragment pairs of A x B, and (quirk) of A u B x the rest
        subs = np.arange(len(self.bin_of))
        SA, SB = subs[inA], subs[inB]
        pairs = [(np.repeat(SA, len(SB)), np.tile(SB, len(SA)), True)]
        if self.quirk:
            S_in, S_out = subs[inA | inB], subs[~(inA | inB)]
            pairs.append((np.repeat(S_in, len(S_out)), np.tile(S_out, len(S_in)), False))
        for sa, sb, is_ab in pairs:
            if len(sa) == 0:
                continue
            old = self.trans(sa, sb, fwd).astype(np.float64)
            new = (self.cis(sa, sb, centre_new) if is_ab else self.trans(sa, sb, fwd_new)).astype(np.float64)
            key = self.bin_of[sa] * self.n + self.bin_of[sb]
            u, inv = np.unique(key, return_inverse=True)
            acc = np.zeros(len(u))
            np.add.at(acc, inv, new - old)          # (in sub-fragment order: the float64 sum of a fragment pair's few terms)
            if not np.isfinite(acc).all():
                bad = True
            t = -np.rint(acc[np.isfinite(acc)] * Q).astype(np.int64)
            total += int(t.sum()); absum += int(np.abs(t).sum())
        return ea, eb, (0 if bad else total), contacts, (NONFINITE if bad else VALID), absum


def dense_loglik(R, state, price_fn):
    """sum_contacts ob * ln(price) - sum over sub-fragment pairs of different bins of price, price_fn(sa, sb) the price array: the
    part of the log-likelihood a layout change can move, summed over EVERY pair (no notion of which pairs changed)."""
    S = len(R.bin_of)
    ia, ib = np.triu_indices(S, 1)
    diff = R.bin_of[ia] != R.bin_of[ib]
    ia, ib = ia[diff], ib[diff]
    keep = R.bin_of[R.row] != R.bin_of[R.col]
    return float((R.count[keep] * np.log(price_fn(R.row[keep], R.col[keep]).astype(np.float64))).sum()
                 - price_fn(ia, ib).astype(np.float64).sum())


def pricer(R, state, centre, fixed=()):
    """price_fn of layout `state` with sub-fragment centres `centre`; pairs with both sub-fragments in one of the masks of `fixed`
    (pairs (mask, centres)) are priced with those centres instead: the pairs a join leaves unchanged, without re-centring."""
    idc = np.asarray(state["id_c"])
    fwd = np.asarray(state["ori"]) == 1
    lab = idc[R.bin_of]

    def price(sa, sb):
        cis = lab[sa] == lab[sb]
        p = np.where(cis, R.cis(sa, sb, centre), R.trans(sa, sb, fwd))
        for mask, cen in fixed:
            m = mask[sa] & mask[sb]
            if m.any():
                p = np.where(m, R.cis(sa, sb, cen), p)
        return p
    return price


def restatement(P, quirk=False):
    return Restatement(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
                       P["param_simu"], P["coo_row"], P["coo_col"], P["coo_val"], quirk=quirk)


PIECES = (6, 1, 4, 9, 2, 5, 3, 7)


def case(name):
    """The junction tests' small problems (tests/junction_reference.py: n_sub 3 ragged with RF counts 1..4 and reversed bins, n_sub 1,
    a ring with RF count 9) with their linear contigs cut into pieces of 1-9 fragments, shuffled, every third piece reversed: many ends
    with contacts between them.  The ring stays a ring."""
    from tests import junction_reference as JR
    P = JR.case(name)
    s = P["S_o_A_frags"]
    lists = contig_lists(s)
    circ = np.asarray(s["circ"])
    rng = np.random.RandomState({"sub3": 1, "sub1": 2, "circ": 3}[name])
    pieces, rings = [], []
    k = 0
    for c, frags in lists.items():
        if circ[frags[0][0]] == 1:
            rings.append(frags)
            continue
        i = 0
        while i < len(frags):
            w = PIECES[k % len(PIECES)]; k += 1
            pieces.append(frags[i:i + w])
            i += w
    order = rng.permutation(len(pieces))
    pieces = [pieces[j] for j in order]
    pieces = [[(f, -o) for f, o in reversed(p)] if j % 3 == 0 else p for j, p in enumerate(pieces)]
    P["S_o_A_frags"] = layout(s["len_bp"], rings + pieces, set(range(len(rings))))
    return P
