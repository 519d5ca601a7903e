"""TEST INFRASTRUCTURE -- numpy restatements of graal_ring_scores and graal_close_rings (graal_amd/csrc/rings.h).

    ring_scores(P, state=None, parts=None)    brute force: every pair of sub-fragments of every contig, one at a time
    ring_scores_windowed(P, state=None, parts=None)   vectorised, fragment pairs enumerated inside the window only (mid-size shapes)
    toggle(state, contig)                     the layout with that contig in the other topology, every coordinate kept
    close(state, frags)                       graal_close_rings: (new layout or None, status words)

The contact model is evaluated operation by operation in float64 and rounded to float32 after each one (rippe_cr of
tests/junction_reference.py, rippe_circ_cr here), as the engine's correctly rounded float32 model does; a term is rounded to Q = 2^30
once (a contact; a fragment pair's mass; a bin's own sub-fragment pairs).  Both return (R int64[n] in Q, contacts int64[n], status
uint8[n], A int64[n] = the sum of |terms| in Q), indexed by fragment, every fragment carrying its contig's values.  parts (a dict) is
filled with per-fragment arrays: 'terms' (the contig's contacts and fragment pairs that were priced, own-bin pairs included),
'contact', 'mass', 'own' (each class's share of R in Q).  Not product code.
"""
import numpy as np

from tests.junction_reference import rippe_cr
from tests.link_reference import rippe_vec
from tests.sim_reference import sub_records

f32 = np.float32
Q = float(1 << 30)
CLOSE, OPEN, SINGLE, NONFINITE = 0, 1, 2, 3
EDIT_OK, EDIT_BAD_FRAG, EDIT_CIRCULAR, EDIT_SINGLE, EDIT_TWICE = range(5)
LIMIT = 2147483648.0      # to_q: a term of 2^31 log-likelihood units or more does not fit


def _pow(x, y):
    with np.errstate(all="ignore"):
        return np.power(np.asarray(x, np.float64), np.float64(y)).astype(np.float32)


def _exp(x):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def rippe_circ_vec(s, s_tot, lin, p):
    """rippe_circ (graal_hip.hip) over arrays, given lin = rippe(s): float64 per operation, rounded to float32 after each one; fmaxf
    returns the other operand for a NaN.  Outside 0 < s < d_max it is v_inter."""
    kuhn, lm, c1, slope, d, d_max, fact, v = [f32(x) for x in p]
    s = np.asarray(s, np.float32); s_tot = np.asarray(s_tot, np.float32); lin = np.asarray(lin, np.float32)
    with np.errstate(all="ignore"):
        K = f32(lm / kuhn)
        nmax = f32(K * f32(1))
        k3 = _pow(kuhn, f32(-3.0))
        norm_circ = ((k3 * _pow(nmax, slope)).astype(np.float32) * _exp(f32(d - f32(2)) / f32(f32(nmax * nmax) + d))).astype(np.float32)
        norm_circ = f32(norm_circ * fact)
        n = (((K * s).astype(np.float32) * (s_tot - s).astype(np.float32)).astype(np.float32) / s_tot).astype(np.float32)
        e = _exp((f32(d - f32(2)) / ((n * n).astype(np.float32) + d).astype(np.float32)).astype(np.float32))
        val = (((k3 * _pow(n, slope)).astype(np.float32) * e).astype(np.float32) * fact).astype(np.float32)
        r = ((val * lin).astype(np.float32) / norm_circ).astype(np.float32)
    r = np.where((s > 0) & (s < d_max), r, f32(0)).astype(np.float32)
    return np.fmax(r, v).astype(np.float32)


def rippe_circ_cr(s, s_tot, p):
    return f32(rippe_circ_vec(np.array([s], np.float32), np.array([s_tot], np.float32), np.array([rippe_cr(s, p)], np.float32), p)[0])


def _q(v):
    return int(np.rint(v * Q))


def _args(P, state):
    return (P["np_sub_frags_id"], P["np_sub_frags_len_bp"], P["np_sub_frags_accu"], P["mean_squared_frags_per_bin"], P["param_simu"],
            P["S_o_A_frags"] if state is None else state, P["coo_row"], P["coo_col"], P["coo_val"])


def _out(n, parts):
    if parts is not None:
        parts.update({k: np.zeros(n, np.int64) for k in ("terms", "contact", "mass", "own")})
    return np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.uint8), np.zeros(n, np.int64)


def _store(m, ring, share, n_terms, absum, wrap, bad, R, Cn, St, A, parts):
    scored = ring or len(m) >= 2
    St[m] = SINGLE if not scored else (NONFINITE if bad else (OPEN if ring else CLOSE))
    R[m] = sum(share.values()) if scored and not bad else 0
    Cn[m] = wrap
    A[m] = absum
    if parts is not None:
        parts["terms"][m] = n_terms
        for k, v in share.items():
            parts[k][m] = v


def ring_scores(P, state=None, parts=None):
    sub_id, sub_len, sub_accu, nfpb, param, state, row, col, count = _args(P, state)
    centre, _, acc, _ = sub_records(sub_id, sub_len, sub_accu, state)
    sid = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    n = len(sid)
    nsub = sid[:, 3]
    bin_of = np.zeros(len(centre), np.int64)
    for b in range(n):
        bin_of[sid[b, :nsub[b]]] = b
    nfpb = f32(nfpb)
    p = [f32(x) for x in param]
    d_max = p[5]
    idc, pos, circ = (np.asarray(state[k]) for k in ("id_c", "pos", "circ"))
    lbp = np.asarray(state["l_cont_bp"])
    row, col, count = np.asarray(row), np.asarray(col), np.asarray(count, dtype=np.float64)
    R, Cn, St, A = _out(n, parts)

    def diff(a, b, s_tot, ring):
        """(in the window, ex_new, ex_old) of sub-fragments a, b"""
        s = f32(abs(f32(centre[b] - centre[a])))
        if not (s > 0 and s < d_max):
            return False, None, None, s
        norm = f32(f32(int(acc[a]) * int(acc[b])) / nfpb)
        lin = rippe_cr(s, p)
        with np.errstate(all="ignore"):
            ex_lin, ex_circ = f32(lin * norm), f32(rippe_circ_cr(s, s_tot, p) * norm)
        return (True, ex_lin, ex_circ, s) if ring else (True, ex_circ, ex_lin, s)

    for c in np.unique(idc):
        m = np.nonzero(idc == c)[0]
        m = m[np.argsort(pos[m])]
        ring = circ[m[0]] == 1
        s_tot = f32(f32(lbp[m[0]]) / f32(1000.0))
        inside = np.zeros(n, bool); inside[m] = True
        share = {"contact": 0, "mass": 0, "own": 0}
        n_terms, absum, wrap, bad = 0, 0, 0, False

        def add(cls, v):
            nonlocal n_terms, absum, bad
            n_terms += 1
            if not np.isfinite(v) or abs(v) >= LIMIT:
                bad = True
                return
            t = _q(v)
            share[cls] += t; absum += abs(t)

        for r, cc, ob in zip(row, col, count):
            if not (inside[bin_of[r]] and inside[bin_of[cc]]):
                continue
            ok, new, old, s = diff(r, cc, s_tot, ring)
            if not ok:
                continue
            with np.errstate(all="ignore"):
                add("contact", ob * (np.log(np.float64(new)) - np.log(np.float64(old))))
            if f32(f32(2) * s) > s_tot:
                wrap += int(np.rint(ob))
        for i, x in enumerate(m):
            for y in m[i:]:
                accm, any_in = 0.0, False
                for ia, a in enumerate(sid[x, :nsub[x]]):
                    for ib, b in enumerate(sid[y, :nsub[y]]):
                        if x == y and ib <= ia:
                            continue
                        ok, new, old, _ = diff(a, b, s_tot, ring)
                        if ok:
                            any_in = True
                            with np.errstate(all="ignore"):
                                accm += np.float64(new) - np.float64(old)
                if any_in:
                    add("own" if x == y else "mass", -accm)
        _store(m, ring, share, n_terms, absum, wrap, bad, R, Cn, St, A, parts)
    return R, Cn, St, A


def ring_scores_windowed(P, state=None, parts=None):
    from tests import window_reference as WR
    sub_id, sub_len, sub_accu, nfpb, param, state, row, col, count = _args(P, state)
    W = WR.Window(sub_id, sub_len, sub_accu, nfpb, param, row, col, count)
    n = W.n
    idc, pos, circ = (np.asarray(state[k], np.int64) for k in ("id_c", "pos", "circ"))
    fwd = np.asarray(state["ori"]) == 1
    start_bp, len_bp = np.asarray(state["start_bp"], np.int64), np.asarray(state["len_bp"], np.int64)
    s_tot_f = (np.asarray(state["l_cont_bp"]).astype(np.float32) / f32(1000.0)).astype(np.float32)
    C = W.centres(np.arange(n), start_bp, fwd)
    d_max = W.d_max
    R, Cn, St, A = _out(n, parts)

    def prices(d, s_tot, aa, ab, ring):
        """(in the window, ex_new, ex_old) per pair"""
        inw = (d > 0) & (d < d_max)
        norm = ((aa * ab).astype(np.float32) / W.nfpb).astype(np.float32)
        lin = rippe_vec(np.where(inw, d, f32(1)).astype(np.float32), W.p)
        with np.errstate(all="ignore"):
            ex_circ = (rippe_circ_vec(np.where(inw, d, f32(1)).astype(np.float32), s_tot, lin, W.p) * norm).astype(np.float32)
            ex_lin = (lin * norm).astype(np.float32)
        return inw, np.where(ring, ex_lin, ex_circ), np.where(ring, ex_circ, ex_lin)

    def rounded(v, present):
        bad = present & (~np.isfinite(v) | (np.abs(v) >= LIMIT))
        t = np.zeros(len(v), np.int64)
        ok = present & ~bad
        t[ok] = np.rint(v[ok] * Q).astype(np.int64)
        return t, bad

    def mass(X, Y, s_tot, ring, own):
        acc = np.zeros(len(X)); present = np.zeros(len(X), bool)
        nx, ny = W.nsub[X], W.nsub[Y]
        for i in range(3):
            for j in range(3):
                if own and j <= i:
                    continue
                k = np.nonzero((i < nx) & (j < ny))[0]
                if len(k) == 0:
                    continue
                x, y = X[k], Y[k]
                inw, new, old = prices(np.abs(C[y, j] - C[x, i]).astype(np.float32), s_tot, W.acc_s[x, i], W.acc_s[y, j], ring)
                with np.errstate(all="ignore"):
                    acc[k] += np.where(inw, new.astype(np.float64) - old.astype(np.float64), 0.0)
                present[k] |= inw
        return rounded(-acc, present) + (present,)

    br, sr = W._sub(W.row)
    bc, sc = W._sub(W.col)
    by_lab = np.where(idc[br] == idc[bc], idc[br], -1)               # a cis contact's contig, sorted once: a slice per contig
    by_order = np.argsort(by_lab, kind="stable")
    by_sorted = by_lab[by_order]
    for lab, m in WR._runs(idc, pos):
        ring = bool(circ[m[0]] == 1)
        s_tot = s_tot_f[m[0]]
        share = {}
        n_terms, absum, bad = 0, 0, False
        # contacts
        k = np.sort(by_order[np.searchsorted(by_sorted, lab, side="left"):np.searchsorted(by_sorted, lab, side="right")])
        a, b = br[k], bc[k]
        d = np.abs(C[b, sc[k]] - C[a, sr[k]]).astype(np.float32)
        inw, new, old = prices(d, s_tot, W.acc_s[a, sr[k]], W.acc_s[b, sc[k]], ring)
        with np.errstate(all="ignore"):
            v = W.count[k] * (np.log(new.astype(np.float64)) - np.log(old.astype(np.float64)))
        t, tb = rounded(v, inw)
        share["contact"] = int(t.sum()); absum += int(np.abs(t).sum()); bad |= bool(tb.any()); n_terms += int(inw.sum())
        wrap = int(np.rint(W.count[k][inw & ((f32(2) * d).astype(np.float32) > s_tot)]).sum())
        # fragment pairs inside the window, then every bin's own pairs
        tot = 0
        for ii, jj, _ in W._window_pairs(start_bp[m], start_bp[m] + len_bp[m]):
            if len(ii) == 0:
                continue
            t, tb, present = mass(m[ii], m[jj], s_tot, ring, False)
            tot += int(t.sum()); absum += int(np.abs(t).sum()); bad |= bool(tb.any()); n_terms += int(present.sum())
        share["mass"] = tot
        t, tb, present = mass(m, m, s_tot, ring, True)
        share["own"] = int(t.sum()); absum += int(np.abs(t).sum()); bad |= bool(tb.any()); n_terms += int(present.sum())
        _store(m, ring, share, n_terms, absum, wrap, bad, R, Cn, St, A, parts)
    return R, Cn, St, A


def _members(state, contig):
    m = np.nonzero(np.asarray(state["id_c"]) == contig)[0]
    return m[np.argsort(np.asarray(state["pos"])[m])]


def toggle(state, contig):
    """The layout with `contig` in the other topology: a linear contig closed (circ 1, head.prev = tail, tail.next = head), a ring opened
    at its wrap (circ 0, the position-0 fragment's prev and the last-position fragment's next -1).  Every other field kept."""
    s = {k: np.array(v, dtype=np.int32, copy=True) for k, v in state.items()}
    m = _members(s, contig)
    head, tail = int(m[0]), int(m[-1])
    if s["circ"][head] == 1:
        s["circ"][m] = 0; s["prev"][head] = -1; s["next"][tail] = -1
    else:
        s["circ"][m] = 1; s["prev"][head] = tail; s["next"][tail] = head
    return s


def with_rings(P, every, seed=None):
    """P with every `every`-th contig of at least 2 fragments (in label order; seeded: a random `1 / every` of them, at least one)
    turned into a ring."""
    s = P["S_o_A_frags"]
    labs = [int(c) for c in np.unique(s["id_c"]) if s["l_cont"][np.nonzero(s["id_c"] == c)[0][0]] >= 2 and
            s["circ"][np.nonzero(s["id_c"] == c)[0][0]] != 1]
    if seed is None:
        pick = labs[::every]
    else:
        pick = list(np.random.RandomState(seed).permutation(labs)[:max(1, len(labs) // every)])
    out = dict(P)
    for c in pick:
        s = toggle(s, c)
    out["S_o_A_frags"] = s
    return out


def close(state, frags):
    """graal_close_rings restated: (the new layout, or None when an entry is refused; the status words)."""
    n = len(state["pos"])
    frags = [int(f) for f in frags]
    st = []
    for f in frags:
        if f < 0 or f >= n:
            st.append(EDIT_BAD_FRAG)
        elif state["circ"][f] == 1:
            st.append(EDIT_CIRCULAR)
        elif state["l_cont"][f] < 2:
            st.append(EDIT_SINGLE)
        else:
            st.append(EDIT_OK)
    named = {}
    for f, r in zip(frags, st):
        if r == EDIT_OK:
            named[int(state["id_c"][f])] = named.get(int(state["id_c"][f]), 0) + 1
    st = [EDIT_TWICE if r == EDIT_OK and named[int(state["id_c"][f])] > 1 else r for f, r in zip(frags, st)]
    if any(r != EDIT_OK for r in st):
        return None, np.array(st, np.int32)
    s = {k: np.array(v, dtype=np.int32, copy=True) for k, v in state.items()}
    for c in named:
        s = toggle(s, c)
    return s, np.array(st, np.int32)
