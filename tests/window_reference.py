"""TEST INFRASTRUCTURE -- windowed, vectorised numpy restatement of graal_junction_scores, graal_end_links and graal_insertions, with the
definitions and roundings of the brute-force restatements (tests/junction_reference.py, link_reference.py, insert_reference.py): the
correctly rounded float32 contact model, a contact's term rounded to Q once, a fragment pair's mass summed over its sub-fragment pairs
in float64 in sub-fragment order (the outer fragment's sub-fragments outer) and rounded to Q once; the same statuses, contact counts and
sums of |terms|.  Fast enough for problems of ~10^4 fragments and ~10^6 contacts.

What makes it fast: a fragment pair's mass is enumerated only where it can be non-zero.  Beyond the contact window (more than
reach_bp = ceil(d_max * 1000) + 1000 bp between the two fragments) the model prices a cis pair at v_inter, exactly the float32 a trans
pair gets, so the pair's new - old is exactly 0 -- except with the trans-branch indexing (quirk) when the lower-id bin of the pair is
reversed and holds sub-fragments of different RF counts: those far pairs are enumerated explicitly, and so are the mirror terms of a
reversed piece of mixed bins against every higher-id bin of a third contig (counted by RF-count pattern: their terms depend on the
pattern alone).  Junction scores come from the pair terms by the prefix-sum identity (a pair (i, j) of positions i < j of a contig
straddles the junctions after positions i .. j - 1); junction_direct() sums a junction over its straddling pairs instead.

Uses tests/sim_reference.py's sub-fragment walk only through its definition (centres of a bin placed at a start in an orientation); no
engine record, slot numbering or kernel output.  Not product code.
"""
import numpy as np

from tests.link_reference import rippe_vec

f32 = np.float32
Q = float(1 << 30)
J_VALID, J_END, J_CIRCULAR, J_NONFINITE = 0, 1, 2, 3
VALID, NONFINITE = 0, 1
CHUNK = 1 << 21                     # fragment pairs per vectorised block
JUNCTION_CLASSES = ("contacts", "near", "wide", "far")


def reach_bp(d_max):
    return int(np.ceil(np.float64(f32(d_max)) * 1000.0)) + 1000


def _runs(idc, pos):
    """Contigs as (label, members in position order) in label order."""
    order = np.lexsort((pos, idc))
    lab = idc[order]
    cut = np.nonzero(np.diff(lab))[0] + 1
    return [(int(g[0]), m) for g, m in zip(np.split(lab, cut), np.split(order, cut))]


class _Acc:
    """The terms of one link or insertion: their sum, the sum of their absolute values, non-finite, and each class's share."""

    def __init__(self):
        self.total, self.absum, self.bad, self.parts = 0, 0, False, {}

    def add_summed(self, cls, total, absum, bad):
        self.total += total; self.absum += absum; self.bad |= bad
        self.parts[cls] = self.parts.get(cls, 0) + total

    def add(self, cls, t, bad):
        self.add_summed(cls, int(t.sum()), int(np.abs(t).sum()), bool(bad.any()))

    def out(self, q, st, a, parts):
        q.append(0 if self.bad else self.total); st.append(NONFINITE if self.bad else VALID); a.append(self.absum)
        if parts is not None:
            parts.append(self.parts)


class Window:
    """Static data of a problem: sub-fragment tables, contacts, parameters, trans-branch indexing on or off."""

    def __init__(self, sub_id, sub_len_kb, sub_accu, nfpb, param, row, col, count, quirk=False):
        sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
        self.n = n = len(sid)
        self.nsub = sid[:, 3].copy()
        self.len_s = np.asarray(sub_len_kb, dtype=np.float32).reshape(-1, 3)
        acc = np.asarray(sub_accu, dtype=np.int64).reshape(-1, 3).copy()
        for w in range(3):
            acc[self.nsub <= w, w] = 0
        self.acc_s = acc
        S = int(self.nsub.sum())
        self.bin_of = np.zeros(S, np.int64)
        self.slot_of = np.zeros(S, np.int64)
        for w in range(3):
            m = self.nsub > w
            self.bin_of[sid[m, w]] = np.nonzero(m)[0]
            self.slot_of[sid[m, w]] = w
        assert all((np.diff(sid[self.nsub == k, :k], axis=1) > 0).all() for k in (2, 3)), "sub-fragment ids in slot order"
        self.last = acc[np.arange(n), self.nsub - 1]
        self.mixed = np.array([len(set(acc[b, :self.nsub[b]].tolist())) > 1 for b in range(n)])
        _, self.pattern = np.unique(np.column_stack([self.nsub, acc]), axis=0, return_inverse=True)   # a bin's RF-count pattern
        self.pattern = self.pattern.reshape(-1)
        self.n_pat = int(self.pattern.max()) + 1
        self.pat_bin = np.zeros(self.n_pat, np.int64)
        self.pat_bin[self.pattern] = np.arange(n)                                       # (a representative bin per pattern)
        self.nfpb = f32(nfpb)
        self.p = [f32(x) for x in param]
        self.v = self.p[7]
        self.d_max = self.p[5]
        self.reach = reach_bp(self.d_max)
        self.row, self.col = np.asarray(row, np.int64), np.asarray(col, np.int64)
        self.count = np.asarray(count, dtype=np.float64)
        self.quirk = quirk

    # ---- prices ------------------------------------------------------------------------------------------------------------------
    def centres(self, bins, start_bp, fwd):
        """float32 [m, 3]: the slot centres (kb) of bins placed at start_bp (bp) in orientation fwd -- the sub-fragment walk."""
        bins = np.asarray(bins, np.int64)
        ns = self.nsub[bins]
        run = (np.asarray(start_bp).astype(np.float32) / f32(1000.0)).astype(np.float32)
        C = np.zeros((len(bins), 3), np.float32)
        rows = np.arange(len(bins))
        for w in range(3):
            ok = w < ns
            slot = np.where(ok, np.where(fwd, w, ns - 1 - w), 0)
            ln = self.len_s[bins, slot]
            c = (run + (ln / f32(2.0)).astype(np.float32)).astype(np.float32)
            C[rows[ok], slot[ok]] = c[ok]
            run = np.where(ok, (run + ln).astype(np.float32), run)
        return C

    def cis(self, aa, ab, d):
        norm = ((aa * ab).astype(np.float32) / self.nfpb).astype(np.float32)
        return (rippe_vec(d, self.p) * norm).astype(np.float32)

    def trans(self, X, Y, aa, ab, fX, fY, low=None):
        if self.quirk:
            low = X < Y if low is None else low
            aa = np.where(low & ~fX, self.last[X], aa)
            ab = np.where(~low & ~fY, self.last[Y], ab)
        return (self.v * ((aa * ab).astype(np.float32) / self.nfpb).astype(np.float32)).astype(np.float32)

    def _price(self, kind, k, x, y, i, j, aa, ab, low):
        if kind[0] == "cis":
            return self.cis(aa, ab, np.abs(kind[2][k, j] - kind[1][k, i]).astype(np.float32))
        return self.trans(x, y, aa, ab, kind[1][k], kind[2][k], None if low is None else low[k])

    def mass(self, X, Y, new, old, low=None):
        """-rint(Q * sum over the sub-fragment pairs of bins X[k] (outer) x Y[k] (inner) of new - old) per pair, and its non-finite flag.
        new / old: ("cis", centres of X [m, 3], centres of Y [m, 3]) or ("trans", fwd of X [m], fwd of Y [m])."""
        X, Y = np.asarray(X, np.int64), np.asarray(Y, np.int64)
        acc = np.zeros(len(X))
        nx, ny = self.nsub[X], self.nsub[Y]
        for i in range(3):
            for j in range(3):
                k = np.nonzero((i < nx) & (j < ny))[0]
                if len(k) == 0:
                    continue
                x, y = X[k], Y[k]
                aa, ab = self.acc_s[x, i], self.acc_s[y, j]
                a = self._price(new, k, x, y, i, j, aa, ab, low).astype(np.float64)
                b = self._price(old, k, x, y, i, j, aa, ab, low).astype(np.float64)
                acc[k] += a - b
        bad = ~np.isfinite(acc)
        t = np.zeros(len(X), np.int64)
        t[~bad] = -np.rint(acc[~bad] * Q).astype(np.int64)
        return t, bad

    def contact_terms(self, ob, new, old, guard=True):
        """rint(Q * ob * (ln new - ln old)) per contact and its non-finite flag (guard: 0 where new == old, as the link restatement)."""
        with np.errstate(all="ignore"):
            v = ob * (np.log(new.astype(np.float64)) - np.log(old.astype(np.float64)))
        if guard:
            v = np.where(new == old, 0.0, v)
        bad = ~np.isfinite(v)
        t = np.zeros(len(v), np.int64)
        t[~bad] = np.rint(v[~bad] * Q).astype(np.int64)
        return t, bad

    def _sub(self, subs):
        return self.bin_of[subs], self.slot_of[subs]

    # ---- junctions -------------------------------------------------------------------------------------------------------------
    def _window_pairs(self, start, end, quirk_mask=None):
        """Position pairs (i, j), i < j, of one contig whose bp gap start[j] - end[i] is <= reach, then (quirk_mask(i, j) given) the far
        pairs it selects; in blocks of about CHUNK pairs."""
        L = len(start)
        jmax = np.searchsorted(start, end + self.reach, side="right") - 1
        jmax = np.maximum(jmax, np.arange(L))
        cnt = jmax - np.arange(L)
        i0 = 0
        while i0 < L:
            tot = np.cumsum(cnt[i0:])
            i1 = i0 + max(1, int(np.searchsorted(tot, CHUNK, side="right")))
            ii = np.repeat(np.arange(i0, i1), cnt[i0:i1])
            first = np.repeat(np.cumsum(cnt[i0:i1]) - cnt[i0:i1], cnt[i0:i1])
            jj = ii + 1 + (np.arange(len(ii)) - first)
            yield ii, jj, False
            i0 = i1
        if quirk_mask is not None:
            for i0 in range(0, L, 256):
                ii, jj = np.meshgrid(np.arange(i0, min(L, i0 + 256)), np.arange(L), indexing="ij")
                far = jj > jmax[ii]
                far &= quirk_mask(ii, jj)
                yield ii[far], jj[far], True

    def _junction_parts(self, state):
        """Per linear contig of >= 2 fragments: (members, [pair terms], contact terms); terms as (lo, hi, term, bad, class): the
        positions lo < hi of the two fragments, the term in Q, its non-finite flag, its index in JUNCTION_CLASSES."""
        idc, pos, circ = (np.asarray(state[k], np.int64) for k in ("id_c", "pos", "circ"))
        fwd = np.asarray(state["ori"]) == 1
        start_bp = np.asarray(state["start_bp"], np.int64)
        len_bp = np.asarray(state["len_bp"], np.int64)
        C = self.centres(np.arange(self.n), start_bp, fwd)
        rm = (~fwd) & self.mixed if self.quirk else None
        br, sr = self._sub(self.row)
        bc, sc = self._sub(self.col)
        same = (idc[br] == idc[bc]) & (br != bc)
        for lab, m in _runs(idc, pos):
            if circ[m[0]] == 1 or len(m) < 2:
                continue
            s, e = start_bp[m], start_bp[m] + len_bp[m]
            qm = None
            if rm is not None and rm[m].any():
                def qm(ii, jj, m=m):
                    x, y = m[ii], m[jj]
                    return rm[np.minimum(x, y)]
            pairs = []
            for ii, jj, far in self._window_pairs(s, e, qm):
                if len(ii) == 0:
                    continue
                X, Y = m[ii], m[jj]
                t, bad = self.mass(X, Y, ("cis", C[X], C[Y]), ("trans", fwd[X], fwd[Y]))
                pairs.append((ii, jj, t, bad, np.where(far, 3, np.where(jj - ii > 64, 2, 1)).astype(np.int8)))
            k = np.nonzero(same & (idc[br] == lab))[0]
            a, b = br[k], bc[k]
            new = self.cis(self.acc_s[a, sr[k]], self.acc_s[b, sc[k]], np.abs(C[b, sc[k]] - C[a, sr[k]]).astype(np.float32))
            old = self.trans(a, b, self.acc_s[a, sr[k]], self.acc_s[b, sc[k]], fwd[a], fwd[b])
            t, bad = self.contact_terms(self.count[k], new, old, guard=False)
            contacts = (np.minimum(pos[a], pos[b]), np.maximum(pos[a], pos[b]), t, bad, np.zeros(len(t), np.int8))
            yield m, pairs, contacts

    def junction_scores(self, state, parts=None):
        """(J int64[n] in Q, status uint8[n], sum of |terms| int64[n] in Q), as tests/junction_reference.junction_scores.  parts (a dict):
        filled with each term class's share of J per fragment -- 'contacts', the mass of pairs 'near' (at most 64 positions apart),
        'wide' (further apart, inside the window) and 'far' (beyond it, priced apart by the trans-branch indexing)."""
        n = self.n
        if parts is not None:
            parts.update({k: np.zeros(n, np.int64) for k in JUNCTION_CLASSES})
        J = np.zeros(n, np.int64)
        A = np.zeros(n, np.int64)
        status = np.full(n, J_END, np.uint8)
        status[np.asarray(state["circ"]) == 1] = J_CIRCULAR
        for m, pairs, contacts in self._junction_parts(state):
            L = len(m)
            D = np.zeros(L + 1, np.int64)
            Da = np.zeros(L + 1, np.int64)
            Db = np.zeros(L + 1, np.int64)
            for lo, hi, t, bad, cls in pairs + [contacts]:
                np.add.at(D, lo, t); np.add.at(D, hi, -t)
                if parts is not None:
                    for k in np.unique(cls):
                        Dk = np.zeros(L + 1, np.int64)
                        sel = cls == k
                        np.add.at(Dk, lo[sel], t[sel]); np.add.at(Dk, hi[sel], -t[sel])
                        parts[JUNCTION_CLASSES[k]][m[:L - 1]] += np.cumsum(Dk)[:L - 1]
                np.add.at(Da, lo, np.abs(t)); np.add.at(Da, hi, -np.abs(t))
                np.add.at(Db, lo, bad.astype(np.int64)); np.add.at(Db, hi, -bad.astype(np.int64))
            j, a, b = (np.cumsum(x)[:L - 1] for x in (D, Da, Db))
            f = m[:L - 1]
            status[f] = np.where(b > 0, J_NONFINITE, J_VALID)
            J[f] = np.where(b > 0, 0, j)
            A[f] = a
        return J, status, A

    def junction_direct(self, state, frags):
        """{f: (J, bad, A)} for the junctions after fragments `frags`, summed directly over the pairs and contacts that straddle them."""
        pos = np.asarray(state["pos"], np.int64)
        idc = np.asarray(state["id_c"], np.int64)
        want = {int(f): [0, False, 0] for f in frags}
        for m, pairs, contacts in self._junction_parts(state):
            here = [f for f in want if idc[f] == idc[m[0]]]
            for f in here:
                k = pos[f]
                for lo, hi, t, bad, _ in pairs + [contacts]:
                    s = (lo <= k) & (k < hi)
                    want[f][0] += int(t[s].sum()); want[f][1] |= bool(bad[s].any()); want[f][2] += int(np.abs(t[s]).sum())
        return {f: (0 if v[1] else v[0], v[1], v[2]) for f, v in want.items()}

    # ---- shared by links and insertions ----------------------------------------------------------------------------------------
    def _layout_tables(self, state):
        idc, pos, circ = (np.asarray(state[k], np.int64) for k in ("id_c", "pos", "circ"))
        len_bp = np.asarray(state["len_bp"], np.int64)
        off = np.zeros(self.n, np.int64)
        members, length = {}, {}
        for lab, m in _runs(idc, pos):
            cs = np.cumsum(len_bp[m])
            off[m] = cs - len_bp[m]
            members[lab], length[lab] = m, int(cs[-1])
        fwd = np.asarray(state["ori"]) == 1
        return idc, circ, len_bp, off, members, length, fwd

    def _contacts_by_label_pair(self, idc):
        br, bc = self.bin_of[self.row], self.bin_of[self.col]
        la, lb = idc[br], idc[bc]
        key = np.minimum(la, lb) * (int(idc.max()) + 1) + np.maximum(la, lb)
        order = np.argsort(key, kind="stable")
        ks = key[order]
        u, first = np.unique(ks, return_index=True)
        last = np.append(first[1:], len(ks))
        return {int(k): order[a:b] for k, a, b in zip(u, first, last)}, int(idc.max()) + 1

    def _touching(self, idc):
        """{label: indices of the contacts with exactly one end in the contig}."""
        br, bc = self.bin_of[self.row], self.bin_of[self.col]
        la, lb = idc[br], idc[bc]
        k = np.nonzero(la != lb)[0]
        lab = np.concatenate([la[k], lb[k]])
        idx = np.concatenate([k, k])
        order = np.argsort(lab, kind="stable")
        lab, idx = lab[order], idx[order]
        u, first = np.unique(lab, return_index=True)
        last = np.append(first[1:], len(lab))
        return {int(x): np.sort(idx[a:b]) for x, a, b in zip(u, first, last)}

    def _contact_prices(self, k, new_start, new_fwd, fwd, kind_new, kind_old, C_old=None):
        """Prices (new, old) of contacts k; new_start / new_fwd: arrays over all bins of the new layout (only the touched ones used)."""
        a, sa = self._sub(self.row[k])
        b, sb = self._sub(self.col[k])
        aa, ab = self.acc_s[a, sa], self.acc_s[b, sb]
        out = []
        for kind, st, fw in ((kind_new, new_start, new_fwd), (kind_old, None, fwd)):
            if kind == "cis":
                if st is None:
                    ca, cb = C_old[a, sa], C_old[b, sb]
                else:
                    ca = self.centres(a, st[a], fw[a])[np.arange(len(a)), sa]
                    cb = self.centres(b, st[b], fw[b])[np.arange(len(b)), sb]
                out.append(self.cis(aa, ab, np.abs(cb - ca).astype(np.float32)))
            else:
                out.append(self.trans(a, b, aa, ab, fw[a], fw[b]))
        return out

    def _pattern_suffix(self, bins):
        """int64 [len(bins), n_pat]: for each of `bins` (sorted), how many of `bins` with a higher id have each RF-count pattern."""
        oh = np.zeros((len(bins), self.n_pat), np.int64)
        oh[np.arange(len(bins)), self.pattern[bins]] = 1
        return np.cumsum(oh[::-1], axis=0)[::-1] - oh

    def _mirror(self, X, fX_new, fX_old, excluded):
        """Terms of the bins X of a reversed piece against every higher-id bin outside `excluded` (the trans-branch indexing re-prices
        those pairs by X's orientation): (sum of terms, sum of |terms|, non-finite)."""
        X = np.asarray(X, np.int64)
        keep = self.mixed[X] & (fX_new != fX_old)
        X, fX_new, fX_old = X[keep], fX_new[keep], fX_old[keep]
        if len(X) == 0:
            return 0, 0, False
        allb = np.arange(self.n)
        cnt_all = self._pattern_suffix(allb)[X]
        ex = np.sort(np.asarray(excluded, np.int64))
        suf = self._pattern_suffix(ex)
        at = np.searchsorted(ex, X)                  # X is in `excluded`: its row there counts the excluded bins above it
        cnt = cnt_all - suf[at]
        P = self.n_pat
        XX = np.repeat(X, P)
        YY = np.tile(self.pat_bin, len(X))
        low = np.ones(len(XX), bool)
        t, bad = self.mass(XX, YY, ("trans", np.repeat(fX_new, P), np.ones(len(XX), bool)),
                           ("trans", np.repeat(fX_old, P), np.ones(len(XX), bool)), low=low)
        c = cnt.reshape(-1)
        used = c > 0
        return int((t[used] * c[used]).sum()), int((np.abs(t[used]) * c[used]).sum()), bool(bad[used].any())

    def _far_quirk(self, X, Y, near, fwd):
        """The far pairs of X x Y (not `near`) whose lower-id bin is reversed and mixed (the trans-branch indexing prices them apart)."""
        lo = np.minimum(X[:, None], Y[None, :])
        m = (~near) & (~fwd[lo]) & self.mixed[lo]
        i, j = np.nonzero(m)
        return i, j

    # ---- links -----------------------------------------------------------------------------------------------------------------
    def link_keys(self, state, min_frags=1):
        """(end_a int64[m], end_b int64[m], contacts int64[m]) of the listed links (an A x B contact inside the window of the canonical
        join), sorted; as tests/link_reference.Restatement.links."""
        idc, circ, len_bp, off, members, length, fwd = self._layout_tables(state)
        elig = {c for c, m in members.items() if circ[m[0]] == 0 and len(m) >= min_frags}
        head = {c: int(m[0]) for c, m in members.items()}
        tail = {c: int(m[-1]) for c, m in members.items()}
        br, sr = self._sub(self.row)
        bc, sc = self._sub(self.col)
        lr, lc = idc[br], idc[bc]
        el = np.zeros(int(idc.max()) + 1, bool)
        el[list(elig)] = True
        k = np.nonzero((lr != lc) & el[lr] & el[lc])[0]
        if len(k) == 0:
            z = np.zeros(0, np.int64)
            return z, z, z
        Lof = np.zeros(len(el), np.int64)
        H = np.zeros(len(el), np.int64)
        T = np.zeros(len(el), np.int64)
        for c in members:
            Lof[c], H[c], T[c] = length[c], head[c], tail[c]
        keys, cnts = [], []
        x, y = br[k], bc[k]
        cx, cy = lr[k], lc[k]
        for sx in (0, 1):
            for sy in (0, 1):
                ex = 2 * np.where(sx, T[cx], H[cx]) + sx
                ey = 2 * np.where(sy, T[cy], H[cy]) + sy
                xa = ex < ey                                  # x's contig is A
                sa = np.where(xa, sx, sy); sb = np.where(xa, sy, sx)
                LA = np.where(xa, Lof[cx], Lof[cy]); LB = np.where(xa, Lof[cy], Lof[cx])

                def place(z, inA):
                    s_ = np.where(inA, sa, sb)
                    keep = np.where(inA, s_ == 1, s_ == 0)
                    o = np.where(keep, off[z], np.where(inA, LA, LB) - off[z] - len_bp[z])
                    return o + np.where(inA, 0, LA), np.where(keep, fwd[z], ~fwd[z])
                stx, fx = place(x, xa)
                sty, fy = place(y, ~xa)
                cxr = self.centres(x, stx, fx)[np.arange(len(x)), sr[k]]
                cyr = self.centres(y, sty, fy)[np.arange(len(y)), sc[k]]
                win = np.abs(cyr - cxr).astype(np.float32) < self.d_max
                keys.append((np.minimum(ex, ey) * (2 * self.n) + np.maximum(ex, ey))[win])
                cnts.append(np.rint(self.count[k][win]))
        keys, cnts = np.concatenate(keys), np.concatenate(cnts)
        u, inv = np.unique(keys, return_inverse=True)
        c = np.zeros(len(u), np.int64)
        np.add.at(c, inv, cnts.astype(np.int64))
        return u // (2 * self.n), u % (2 * self.n), c

    def link_scores(self, state, ea_list, eb_list, parts=None):
        """(q int64[m] in Q, status uint8[m], sum of |terms| int64[m] in Q) of the links (ea, eb), ea < eb, listed or not.  parts (a
        list): one dict per link of each term class's share of q -- 'contacts' (A x B), 'contacts_rest' (A u B x the rest, indexing
        only), 'mass' (A x B inside the window), 'far' (beyond it, indexing only), 'mirror' (a reversed contig's mixed bins against the
        higher-id bins of the rest, indexing only)."""
        idc, circ, len_bp, off, members, length, fwd = self._layout_tables(state)
        bylab, nl = self._contacts_by_label_pair(idc)
        touch = self._touching(idc) if self.quirk else None
        out_q, out_st, out_a = [], [], []
        for ea, eb in zip(ea_list, eb_list):
            ea, eb = int(ea), int(eb)
            ca, cb = int(idc[ea >> 1]), int(idc[eb >> 1])
            sa, sb = ea & 1, eb & 1
            MA, MB = members[ca], members[cb]
            LA, LB = length[ca], length[cb]
            st = np.zeros(self.n, np.int64)
            fn = fwd.copy()
            st[MA] = off[MA] if sa == 1 else LA - off[MA] - len_bp[MA]
            fn[MA] = fwd[MA] if sa == 1 else ~fwd[MA]
            st[MB] = LA + (off[MB] if sb == 0 else LB - off[MB] - len_bp[MB])
            fn[MB] = fwd[MB] if sb == 0 else ~fwd[MB]
            acc = _Acc()
            # contacts: A x B (trans -> cis); with the indexing, A u B x the rest (trans -> trans)
            k = bylab.get(min(ca, cb) * nl + max(ca, cb), np.zeros(0, np.int64))
            groups = [(k, "cis", "contacts")]
            if self.quirk:
                ks = np.union1d(touch.get(ca, np.zeros(0, np.int64)), touch.get(cb, np.zeros(0, np.int64)))
                groups.append((np.setdiff1d(ks, k), "trans", "contacts_rest"))
            for kk, kind, cls in groups:
                if len(kk) == 0:
                    continue
                new, old = self._contact_prices(kk, st, fn, fwd, kind, "trans")
                acc.add(cls, *self.contact_terms(self.count[kk], new, old))
            # mass: A x B inside the window (and the far pairs the indexing prices apart), A outer
            gA = LA - (st[MA] + len_bp[MA])
            gB = st[MB] - LA
            wa, wb = np.nonzero(gA <= self.reach)[0], np.nonzero(gB <= self.reach)[0]
            near_ab = (gA[wa][:, None] + gB[wb][None, :]) <= self.reach
            i, j = np.nonzero(near_ab)
            sets = [(MA[wa[i]], MB[wb[j]], "mass")]
            if self.quirk:
                near = np.zeros((len(MA), len(MB)), bool)
                near[np.ix_(wa, wb)] = near_ab
                fi, fj = self._far_quirk(MA, MB, near, fwd)
                sets.append((MA[fi], MB[fj], "far"))
            for X, Y, cls in sets:
                if len(X):
                    CX = self.centres(X, st[X], fn[X]); CY = self.centres(Y, st[Y], fn[Y])
                    acc.add(cls, *self.mass(X, Y, ("cis", CX, CY), ("trans", fwd[X], fwd[Y])))
            if self.quirk:
                AB = np.concatenate([MA, MB])
                for M in (MA, MB):
                    acc.add_summed("mirror", *self._mirror(M, fn[M], fwd[M], AB))
            acc.out(out_q, out_st, out_a, parts)
        return np.array(out_q, np.int64), np.array(out_st, np.uint8), np.array(out_a, np.int64)

    def links(self, state, min_frags=1):
        """The whole table: (end_a, end_b, q, contacts, status, sum of |terms|), as tests/link_reference.Restatement.links."""
        a, b, c = self.link_keys(state, min_frags)
        q, st, A = self.link_scores(state, a, b)
        return a, b, q, c, st, A

    # ---- insertions ------------------------------------------------------------------------------------------------------------
    def insertion_keys(self, state, max_piece_frags=1):
        """(piece, after, rev, contacts) of the listed insertions (a P x T contact inside the window of the inserted layout), sorted
        by (after, piece, rev); as tests/insert_reference.Restatement.insertions."""
        idc, circ, len_bp, off, members, length, fwd = self._layout_tables(state)
        nl = int(idc.max()) + 1
        lin = np.zeros(nl, bool); piece = np.zeros(nl, bool)
        for c, m in members.items():
            lin[c] = circ[m[0]] == 0
            piece[c] = lin[c] and len(m) <= max_piece_frags
        br, sr = self._sub(self.row)
        bc, sc = self._sub(self.col)
        keys, cnts = [], []
        for (x, sx, y, sy) in ((br, sr, bc, sc), (bc, sc, br, sr)):    # x in the piece P, y in the target T
            cx, cy = idc[x], idc[y]
            k = np.nonzero((cx != cy) & piece[cx] & lin[cy])[0]
            for c_t in np.unique(cy[k]):
                MT = members[int(c_t)]
                if len(MT) < 2:
                    continue
                E = off[MT[:-1]] + len_bp[MT[:-1]]                    # the junction after position i sits at E[i]
                kk = k[cy[k] == c_t]
                yy = y[kk]
                lo = np.searchsorted(E, off[yy] - self.reach, side="left")
                hi = np.searchsorted(E, off[yy] + len_bp[yy] + self.reach, side="right")
                n_j = hi - lo
                ci = np.repeat(kk, n_j)
                ji = np.repeat(lo, n_j) + (np.arange(n_j.sum()) - np.repeat(np.cumsum(n_j) - n_j, n_j))
                for rev in (0, 1):
                    xs, ys = x[ci], y[ci]
                    cp = idc[xs]
                    MPh = np.array([members[int(c)][0] for c in cp], np.int64)
                    LP = np.array([length[int(c)] for c in cp], np.int64)
                    Ej = E[ji]
                    px = Ej + np.where(rev == 0, off[xs], LP - off[xs] - len_bp[xs])
                    fx = fwd[xs] if rev == 0 else ~fwd[xs]
                    posy = np.asarray(state["pos"], np.int64)[ys]
                    in1 = posy <= ji
                    py = off[ys] + np.where(in1, 0, LP)
                    cxr = self.centres(xs, px, fx)[np.arange(len(xs)), sx[ci]]
                    cyr = self.centres(ys, py, fwd[ys])[np.arange(len(ys)), sy[ci]]
                    win = np.abs(cyr - cxr).astype(np.float32) < self.d_max
                    after = MT[ji]
                    keys.append(((after * self.n + MPh) * 2 + rev)[win])
                    cnts.append(np.rint(self.count[ci][win]))
        if not keys:
            z = np.zeros(0, np.int64)
            return z, z, z, z
        keys, cnts = np.concatenate(keys), np.concatenate(cnts)
        u, inv = np.unique(keys, return_inverse=True)
        c = np.zeros(len(u), np.int64)
        np.add.at(c, inv, cnts.astype(np.int64))
        rev = u % 2
        return (u // 2) % self.n, (u // 2) // self.n, rev, c

    def insertion_scores(self, state, pieces, afters, revs, parts=None):
        """(q int64[m] in Q, status uint8[m], sum of |terms| int64[m] in Q) of the insertions (piece head, after, rev).  parts (a
        list): one dict per insertion of each term class's share of q -- 'contacts' (P x T), 'contacts_t12' (T1 x T2), 'contacts_rest'
        (P x the rest, indexing only), 'mass' (P x T inside the window), 'far' (P x T beyond it, indexing only), 't12' (T1 x T2),
        'mirror' (a reversed piece's mixed bins against the higher-id bins of the rest, indexing only)."""
        idc, circ, len_bp, off, members, length, fwd = self._layout_tables(state)
        pos = np.asarray(state["pos"], np.int64)
        C_old = self.centres(np.arange(self.n), np.asarray(state["start_bp"], np.int64), fwd)
        bylab, nl = self._contacts_by_label_pair(idc)
        touch = self._touching(idc) if self.quirk else None
        out_q, out_st, out_a = [], [], []
        for head, f, rev in zip(pieces, afters, revs):
            head, f, rev = int(head), int(f), int(rev)
            cp, ct = int(idc[head]), int(idc[f])
            MP, MT = members[cp], members[ct]
            LP = length[cp]
            E = int(off[f] + len_bp[f])
            in1 = pos[MT] <= pos[f]
            T1, T2 = MT[in1], MT[~in1]
            st = np.zeros(self.n, np.int64)
            fn = fwd.copy()
            st[MT] = off[MT] + np.where(in1, 0, LP)
            st[MP] = E + (off[MP] if rev == 0 else LP - off[MP] - len_bp[MP])
            fn[MP] = fwd[MP] if rev == 0 else ~fwd[MP]
            acc = _Acc()
            # contacts: P x T (trans -> cis), T1 x T2 (cis -> cis), with the indexing P x the rest (trans -> trans)
            kpt = bylab.get(min(cp, ct) * nl + max(cp, ct), np.zeros(0, np.int64))
            kt = bylab.get(ct * nl + ct, np.zeros(0, np.int64))
            a, b = self.bin_of[self.row[kt]], self.bin_of[self.col[kt]]
            t1 = np.zeros(self.n, bool); t1[T1] = True
            t2 = np.zeros(self.n, bool); t2[T2] = True
            k12 = kt[(t1[a] & t2[b]) | (t2[a] & t1[b])]
            groups = [(kpt, "cis", "trans", "contacts"), (k12, "cis", "cis", "contacts_t12")]
            if self.quirk:
                kr = touch.get(cp, np.zeros(0, np.int64))
                groups.append((np.setdiff1d(kr, kpt), "trans", "trans", "contacts_rest"))
            for kk, kn, ko, cls in groups:
                if len(kk) == 0:
                    continue
                new, old = self._contact_prices(kk, st, fn, fwd, kn, ko, C_old)
                acc.add(cls, *self.contact_terms(self.count[kk], new, old))
            # mass: P x T (P outer) inside the window and the indexing's far pairs; T1 x T2 (T1 outer) inside the old window
            gT = np.where(in1, E - (off[MT] + len_bp[MT]), off[MT] - E)
            wt = np.nonzero(gT <= self.reach)[0]
            sets = [(np.repeat(MP, len(wt)), np.tile(MT[wt], len(MP)), "mass")]
            if self.quirk:
                near = np.zeros((len(MP), len(MT)), bool)
                near[:, wt] = True
                fi, fj = self._far_quirk(MP, MT, near, fwd)
                sets.append((MP[fi], MT[fj], "far"))
            for X, Y, cls in sets:
                if len(X):
                    acc.add(cls, *self.mass(X, Y, ("cis", self.centres(X, st[X], fn[X]), self.centres(Y, st[Y], fn[Y])),
                                            ("trans", fwd[X], fwd[Y])))
            g1 = E - (off[T1] + len_bp[T1])
            g2 = off[T2] - E
            w1, w2 = np.nonzero(g1 <= self.reach)[0], np.nonzero(g2 <= self.reach)[0]
            i, j = np.nonzero(g1[w1][:, None] + g2[w2][None, :] <= self.reach)
            X, Y = T1[w1[i]], T2[w2[j]]
            if len(X):
                acc.add("t12", *self.mass(X, Y, ("cis", self.centres(X, st[X], fn[X]), self.centres(Y, st[Y], fn[Y])),
                                          ("cis", C_old[X], C_old[Y])))
            if self.quirk:
                acc.add_summed("mirror", *self._mirror(MP, fn[MP], fwd[MP], np.concatenate([MP, MT])))
            acc.out(out_q, out_st, out_a, parts)
        return np.array(out_q, np.int64), np.array(out_st, np.uint8), np.array(out_a, np.int64)

    def insertions(self, state, max_piece_frags=1):
        """The whole table: (piece, after, rev, q, contacts, status, sum of |terms|), as tests/insert_reference.Restatement.insertions."""
        p, f, r, c = self.insertion_keys(state, max_piece_frags)
        q, st, A = self.insertion_scores(state, p, f, r)
        return p, f, r, q, c, st, A


def window(P, quirk=False):
    return Window(P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"],
                  P["param_simu"], P["coo_row"], P["coo_col"], P["coo_val"], quirk=quirk)
