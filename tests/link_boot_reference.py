"""TEST INFRASTRUCTURE -- numpy restatement of graal_end_links_bootstrap (graal_amd/csrc/links_boot.h): the Poisson bootstrap of the
contacts behind every listed link.  Built on tests/link_reference.py (the prices, the joined layouts, the listed set), on
tests/sim_reference.py (the Philox counters, the uniform stream, the Poisson sampler and its near-a-boundary flag, through
tests/junction_boot_reference.draw_counts: the junction bootstrap's draws ARE the link bootstrap's) and, for its own check
(tests/test_links_bootstrap_cpu.py), on link_reference's links(): with the count itself for the draw it is L exactly.

    L*_r(link) = mass(link) + sum over the contacts k the link re-prices of rint(Q * draw_{k,r} * (ln new_k - ln old_k)),
    draw_{k,r} = poisson(ob_k, Stream(row_k, col_k, 2 | r << 8, seed)),

the contacts a link re-prices those of link_reference._link: the contacts between its two contigs (trans now, cis after the join) and,
with the indexing mode on, the contacts between the two contigs and every other fragment (trans in both layouts).  mass(link): the
expected-mass terms of link_reference._link, which multiply no count.

A draw whose uniform came within 1e-6 (relative) of a boundary it was compared with is FLAGGED: the GPU's exp / ln round differently
from libm in the last place and may tip it.  A flagged draw excuses the (link, replicate) cells whose sum holds a non-zero term of that
contact, nothing else.  Not product code."""
import numpy as np

from tests import junction_boot_reference as BR
from tests import link_reference as LR
from tests.sim_reference import sub_records

Q = LR.Q
VALID = LR.VALID


class LinkBoot:
    """The listed links of one layout of one problem: the mass part, the statuses and every re-priced contact's unit term, once;
    replicates on demand.  R: a link_reference.Restatement (its quirk flag is the mode)."""

    def __init__(self, R, state, min_frags=1):
        self.R = R
        ends = LR.ends_of(state, min_frags)
        fwd = np.asarray(state["ori"]) == 1
        idc = np.asarray(state["id_c"])
        lab_sub = idc[R.bin_of]
        d_max = R.p[5]
        E = sorted(ends)
        rows = []
        for i, ea in enumerate(E):
            for eb in E[i + 1:]:
                if ends[ea] != ends[eb]:
                    u = self._units(state, ea, eb, ends[ea], ends[eb], fwd, lab_sub, d_max)
                    if u is not None:
                        rows.append((ea, eb) + u)
        self.m = len(rows)
        self.end_a = np.array([x[0] for x in rows], np.int64)
        self.end_b = np.array([x[1] for x in rows], np.int64)
        self.sel = [x[2] for x in rows]                       # per link: indices into the contact list
        self.t = [x[3] for x in rows]                         # per link: the unit terms ln new - ln old (0 where new == old)
        self.mass = np.array([x[4] for x in rows], np.int64)
        self.A_mass = np.array([x[5] for x in rows], np.int64)
        self.bad_mass = np.array([x[6] for x in rows], bool)
        self.in_win = [x[7] for x in rows]                    # per link: which of its contacts count as evidence
        self.used = np.zeros(len(R.row), bool)                # contacts with a non-zero unit in some link
        for s, t in zip(self.sel, self.t):
            self.used[s[t != 0.0]] = True

    def _units(self, state, ea, eb, ca, cb, fwd, lab_sub, d_max):
        """link_reference.Restatement._link with the count left out of the contact terms."""
        R = self.R
        J = LR.join_layout(state, ea, eb)
        centre_new, _, _, _ = sub_records(R.sub_id, R.sub_len_kb, R.sub_accu, J)
        fwd_new = np.asarray(J["ori"]) == 1
        inA, inB = lab_sub == ca, lab_sub == cb
        r, c = R.row, R.col
        ab = (inA[r] & inB[c]) | (inB[r] & inA[c])
        out_ = (inA[r] | inB[r]) != (inA[c] | inB[c])
        if not ab.any():
            return None
        sd = np.abs(centre_new[c] - centre_new[r]).astype(np.float32)
        in_win = ab & (sd < d_max)
        if not in_win.any():
            return None
        sel = ab | (out_ if R.quirk else np.zeros_like(ab))
        idx = np.nonzero(sel)[0]
        rs, cs = r[idx], c[idx]
        old = R.trans(rs, cs, fwd)
        new = np.where(ab[idx], R.cis(rs, cs, centre_new), R.trans(rs, cs, fwd_new))
        with np.errstate(all="ignore"):
            t = np.log(new.astype(np.float64)) - np.log(old.astype(np.float64))
        t = np.where(new == old, 0.0, t)
        total, absum, bad = 0, 0, False
        subs = np.arange(len(R.bin_of))
        SA, SB = subs[inA], subs[inB]
        pairs = [(np.repeat(SA, len(SB)), np.tile(SB, len(SA)), True)]
        if R.quirk:
            S_in, S_out = subs[inA | inB], subs[~(inA | inB)]
            pairs.append((np.repeat(S_in, len(S_out)), np.tile(S_out, len(S_in)), False))
        for sa, sb, is_ab in pairs:
            if len(sa) == 0:
                continue
            o = R.trans(sa, sb, fwd).astype(np.float64)
            n = (R.cis(sa, sb, centre_new) if is_ab else R.trans(sa, sb, fwd_new)).astype(np.float64)
            key = R.bin_of[sa] * R.n + R.bin_of[sb]
            u, inv = np.unique(key, return_inverse=True)
            acc = np.zeros(len(u))
            np.add.at(acc, inv, n - o)
            if not np.isfinite(acc).all():
                bad = True
            q = -np.rint(acc[np.isfinite(acc)] * Q).astype(np.int64)
            total += int(q.sum()); absum += int(np.abs(q).sum())
        return idx, t, total, absum, bad, in_win[idx]

    def score(self, counts):
        """(L int64[m], sum of |terms| int64[m], status uint8[m]) with contact k of the list counting counts[k]."""
        counts = np.asarray(counts, np.float64)
        L = np.zeros(self.m, np.int64)
        A = np.zeros(self.m, np.int64)
        st = np.zeros(self.m, np.uint8)
        for i in range(self.m):
            with np.errstate(all="ignore"):
                v = counts[self.sel[i]] * self.t[i]
            v = np.where(self.t[i] == 0.0, 0.0, v)
            fin = np.isfinite(v)
            q = np.rint(v[fin] * Q).astype(np.int64)
            bad = self.bad_mass[i] or not fin.all()
            L[i] = 0 if bad else self.mass[i] + int(q.sum())
            A[i] = self.A_mass[i] + int(np.abs(q).sum())
            st[i] = LR.NONFINITE if bad else VALID
        return L, A, st

    def contact_part(self, counts):
        """float64[m]: the contact part of every link in log-likelihood units, unrounded."""
        counts = np.asarray(counts, np.float64)
        return np.array([float((counts[s] * t)[t != 0.0].sum()) for s, t in zip(self.sel, self.t)])

    def contact_var(self):
        """float64[m]: sigma^2 = sum of ob * t^2, the variance of the contact part under the Poisson bootstrap."""
        ob = self.R.count
        return np.array([float((ob[s] * t * t)[t != 0.0].sum()) for s, t in zip(self.sel, self.t)])

    def draws(self, seed, r):
        """(count float64[nnz], flagged bool[nnz]) of replicate r: drawn for the contacts some link re-prices, the others keep 0 / False
        (no link reads them)."""
        R = self.R
        k = np.nonzero(self.used)[0]
        c = np.zeros(len(R.row), np.float64)
        f = np.zeros(len(R.row), bool)
        ck, fk = BR.draw_counts(R.row[k], R.col[k], R.count[k], seed, r)
        c[k], f[k] = ck, fk
        return c, f

    def replicate(self, seed, r):
        """(L*_r int64[m], sum of |terms| int64[m], flagged bool[m], status uint8[m]) of replicate r."""
        c, f = self.draws(seed, r)
        L, A, st = self.score(c)
        fl = np.array([bool(f[s[t != 0.0]].any()) for s, t in zip(self.sel, self.t)], bool)
        return L, A, fl, st

    def replicates(self, seed, reps):
        out = [self.replicate(seed, r) for r in reps]
        return tuple(np.stack([o[i] for o in out]) for i in range(4))


def best_partners(end_a, end_b, row, valid):
    """{end: partner} under the scores `row`: every end's best partner among the valid links, ties towards the lower partner end."""
    a, b = np.asarray(end_a, np.int64), np.asarray(end_b, np.int64)
    ok = np.nonzero(np.asarray(valid, bool))[0]
    end = np.concatenate([a[ok], b[ok]])
    other = np.concatenate([b[ok], a[ok]])
    s = np.concatenate([np.asarray(row, np.int64)[ok]] * 2)
    order = np.lexsort((other, -s, end))
    e, o = end[order], other[order]
    first = np.concatenate([[True], e[1:] != e[:-1]]) if len(e) else np.zeros(0, bool)
    return dict(zip(e[first].tolist(), o[first].tolist()))


def mutual_counts(end_a, end_b, q_rep, valid, threshold=0):
    """int64[m]: in how many rows of q_rep [R, m] a link is mutual -- its score above the threshold and each of its two ends the other's
    best partner among the valid links under that row's scores, ties towards the lower partner end (graal_end_links_best's rule)."""
    a, b = np.asarray(end_a, np.int64), np.asarray(end_b, np.int64)
    ok = np.nonzero(np.asarray(valid, bool))[0]
    out = np.zeros(len(a), np.int64)
    for row in np.asarray(q_rep, np.int64):
        best = best_partners(a, b, row, valid)
        for k in ok:
            if row[k] > threshold and best.get(int(a[k])) == int(b[k]) and best.get(int(b[k])) == int(a[k]):
                out[k] += 1
    return out


# ---- the cases the CPU and GPU tests share ------------------------------------------------------------------------------------------
# tests/test_links_gpu.py's cases (link_reference.case, quirk, min_frags), each with a resampling seed
SMALL_CASES = (("sub3", False, 1, 7), ("sub3", True, 1, 7), ("sub3", True, 3, 8), ("sub1", False, 1, 8), ("sub1", False, 4, 9),
               ("circ", False, 1, 9), ("circ", True, 2, 10))
N_REP = 150                             # three batches of the engine's 64, the last one short
REF_REPS = (0, 1, 2, 63, 64, 128, 149)  # restated: the first ones, both sides of every batch boundary, the last
DEFINING_REPS = (0, 64, 149)            # replayed through graal_end_links on a fresh engine
PLANTED = BR.PLANTED                    # counts for the sampler's branch above 10
FILL = BR.FILL                          # a non-integer count: the rate as it stands, float32(1.7)
MID_SEED, MID_REPS, MID_MIN_FRAGS = 12, 8, 1
_CACHE = {}


def small_case(name):
    """link_reference.case(name) with float32 counts, six of them replaced by PLANTED and one by FILL, each on a contact with a non-zero
    unit term in a listed link (min_frags 1, indexing mode off)."""
    if name not in _CACHE:
        P = LR.case(name)
        B = LinkBoot(LR.restatement(P), P["S_o_A_frags"], 1)
        inside = np.zeros(len(B.used), bool)
        for s, t, w in zip(B.sel, B.t, B.in_win):
            inside[s[(t != 0.0) & np.isfinite(t) & w]] = True
        k = np.nonzero(inside)[0]
        assert len(k) >= len(PLANTED) + 1, len(k)
        pick = k[np.linspace(0, len(k) - 1, len(PLANTED) + 1).astype(int)]
        assert len(set(pick.tolist())) == len(pick)
        v = np.asarray(P["coo_val"]).astype(np.float32)
        v[pick[:-1]] = PLANTED
        v[pick[-1]] = FILL
        P["coo_val"] = v
        _CACHE[name] = P
    return _CACHE[name]


def small_boot(name, quirk, min_frags):
    key = (name, quirk, min_frags)
    if key not in _CACHE:
        P = small_case(name)
        _CACHE[key] = LinkBoot(LR.restatement(P, quirk=quirk), P["S_o_A_frags"], min_frags)
    return _CACHE[key]


def small_replicates(name, quirk, min_frags, seed):
    key = (name, quirk, min_frags, seed)
    if key not in _CACHE:
        _CACHE[key] = small_boot(name, quirk, min_frags).replicates(seed, REF_REPS)
    return _CACHE[key]


# ---- mid size: the same on tests/window_reference.py's windowed restatement ------------------------------------------------------------
class WindowLinkBoot:
    """LinkBoot's interface over a window_reference.Window: the listed links (link_keys), the part of every score that multiplies no
    count (link_scores on a list of zero counts: mass, far pairs, mirrors), and per link the contacts it re-prices with their unit terms
    -- link_scores' own selection (A x B; with the indexing mode, A u B against the rest) and prices."""

    def __init__(self, W, state, min_frags=1):
        import copy
        self.W = W
        self.end_a, self.end_b, _ = W.link_keys(state, min_frags)
        self.m = len(self.end_a)
        W0 = copy.copy(W)
        W0.count = np.zeros(len(W.count), np.float64)
        self.mass, st, self.A_mass = W0.link_scores(state, self.end_a, self.end_b)
        self.bad_mass = st != VALID
        idc, circ, len_bp, off, members, length, fwd = W._layout_tables(state)
        bylab, nl = W._contacts_by_label_pair(idc)
        touch = W._touching(idc) if W.quirk else None
        none = np.zeros(0, np.int64)
        self.sel, self.t = [], []
        for ea, eb in zip(self.end_a.tolist(), self.end_b.tolist()):
            ca, cb = int(idc[ea >> 1]), int(idc[eb >> 1])
            sa, sb = ea & 1, eb & 1
            MA, MB = members[ca], members[cb]
            LA, LB = length[ca], length[cb]
            st_ = np.zeros(W.n, np.int64)
            fn = fwd.copy()
            st_[MA] = off[MA] if sa == 1 else LA - off[MA] - len_bp[MA]
            fn[MA] = fwd[MA] if sa == 1 else ~fwd[MA]
            st_[MB] = LA + (off[MB] if sb == 0 else LB - off[MB] - len_bp[MB])
            fn[MB] = fwd[MB] if sb == 0 else ~fwd[MB]
            k = bylab.get(min(ca, cb) * nl + max(ca, cb), none)
            groups = [(k, "cis")]
            if W.quirk:
                groups.append((np.setdiff1d(np.union1d(touch.get(ca, none), touch.get(cb, none)), k), "trans"))
            ks, ts = [], []
            for kk, kind in groups:
                if len(kk):
                    new, old = W._contact_prices(kk, st_, fn, fwd, kind, "trans")
                    with np.errstate(all="ignore"):
                        t = np.log(new.astype(np.float64)) - np.log(old.astype(np.float64))
                    t = np.where(new == old, 0.0, t)
                    ks.append(kk[t != 0.0]); ts.append(t[t != 0.0])
            self.sel.append(np.concatenate(ks) if ks else none)
            self.t.append(np.concatenate(ts) if ts else np.zeros(0))
        self.used = np.zeros(len(W.row), bool)
        for s in self.sel:
            self.used[s] = True

    def score(self, counts):
        counts = np.asarray(counts, np.float64)
        L = np.zeros(self.m, np.int64)
        A = np.zeros(self.m, np.int64)
        st = np.zeros(self.m, np.uint8)
        for i in range(self.m):
            with np.errstate(all="ignore"):
                v = counts[self.sel[i]] * self.t[i]
            fin = np.isfinite(v)
            q = np.rint(v[fin] * Q).astype(np.int64)
            bad = bool(self.bad_mass[i]) or not fin.all()
            L[i] = 0 if bad else self.mass[i] + int(q.sum())
            A[i] = self.A_mass[i] + int(np.abs(q).sum())
            st[i] = LR.NONFINITE if bad else VALID
        return L, A, st

    def replicate(self, seed, r):
        W = self.W
        k = np.nonzero(self.used)[0]
        c = np.zeros(len(W.row), np.float64)
        f = np.zeros(len(W.row), bool)
        c[k], f[k] = BR.draw_counts(W.row[k], W.col[k], W.count[k], seed, r)
        L, A, st = self.score(c)
        return L, A, np.array([bool(f[s].any()) for s in self.sel], bool), st

    def replicates(self, seed, reps):
        out = [self.replicate(seed, r) for r in reps]
        return tuple(np.stack([o[i] for o in out]) for i in range(4))


def mid_replicates(quirk):
    """(WindowLinkBoot, its MID_REPS replicates under MID_SEED) of junction_boot_reference.mid_case() in its own layout."""
    key = ("m2", quirk)
    if key not in _CACHE:
        from tests import window_reference as WR
        P = BR.mid_case()
        B = WindowLinkBoot(WR.window(P, quirk), P["S_o_A_frags"], MID_MIN_FRAGS)
        _CACHE[key] = (B, B.replicates(MID_SEED, range(MID_REPS)))
    return _CACHE[key]
