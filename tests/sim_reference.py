"""TEST INFRASTRUCTURE -- numpy restatement of graal_simulate_contacts (graal_amd/csrc/simulate.h): the same Philox4x32-10 counters, the
same draws in the same double-precision operation order.  Where the two can still differ -- the GPU's exp / log (model_math.h) and the
float32 pow / exp of the contact model round differently from libm in the last place -- the reference FLAGS the draw: a uniform within
1e-6 relative of the boundary it was compared with.  A flagged window pair may differ; a flagged background chunk may differ as a whole
(one tipped decision shifts the rest of its stream).  A background skip g = -ln(u) / Lmax is flagged near an integer >= 1 and near the
chunk's remaining width only: g > 0 always, so floor(g) = 0 cannot tip at 0, and flagging there (as an earlier version did) excused
almost every chunk of a row with a large Lmax.  That makes the reference stricter, never laxer.  Not product code."""
import math

import numpy as np

from oracle.sparse_numpy import rippe_f32, rippe_circ_f32

f32 = np.float32
M32 = 0xFFFFFFFF
CHUNK = 4096          # simulate.h: SIM_CHUNK
KMAX = 256            # SIM_KMAX
TRIES = 64            # SIM_TRIES
PTRS_MIN = 10.0       # SIM_PTRS_MIN
TOL = 1e-6
SKIP_TOL = 1e-9


# ---- Philox (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11)
_P32 = dict(M=(0xD2511F53, 0xCD9E8D57), W=(0x9E3779B9, 0xBB67AE85), bits=32)
_P64 = dict(M=(0xD2E7470EE14C6C93, 0xCA5A826395121157), W=(0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B), bits=64)


def philox_scalar(ctr, key, width=32, rounds=10):
    """Philox4xW-R on Python ints (W = 32 or 64): ctr = 4 words, key = 2 words."""
    P = _P32 if width == 32 else _P64
    mask = (1 << P["bits"]) - 1
    c = [int(x) & mask for x in ctr]
    k0, k1 = int(key[0]) & mask, int(key[1]) & mask
    for r in range(rounds):
        if r:
            k0 = (k0 + P["W"][0]) & mask
            k1 = (k1 + P["W"][1]) & mask
        p0 = P["M"][0] * c[0]
        p1 = P["M"][1] * c[2]
        c = [((p1 >> P["bits"]) ^ c[1] ^ k0) & mask, p1 & mask, ((p0 >> P["bits"]) ^ c[3] ^ k1) & mask, p0 & mask]
    return c


def philox4x32(c0, c1, c2, c3, seed):
    """Vectorised Philox4x32-10: counters are arrays (broadcast), key = (seed low word, seed high word).  Returns 4 uint64 arrays of words."""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(M32) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.uint64(seed & M32), np.uint64((seed >> 32) & M32)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    mask, sh = np.uint64(M32), np.uint64(32)
    for r in range(10):
        if r:
            k0 = (k0 + w0) & mask
            k1 = (k1 + w1) & mask
        p0 = m0 * c[0]
        p1 = m1 * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & mask, (p0 >> sh) ^ c[3] ^ k1, p0 & mask]
    return c


def uniforms_from_words(w):
    """The two uniforms of one counter: ((w1 w0) >> 12 + 0.5) 2^-52, ((w3 w2) >> 12 + 0.5) 2^-52."""
    x0 = (np.asarray(w[1], dtype=np.uint64) << np.uint64(32)) | np.asarray(w[0], dtype=np.uint64)
    x1 = (np.asarray(w[3], dtype=np.uint64) << np.uint64(32)) | np.asarray(w[2], dtype=np.uint64)
    u0 = ((x0 >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    u1 = ((x1 >> np.uint64(12)).astype(np.float64) + 0.5) * 2.0 ** -52
    return u0, u1


class Stream:
    """The uniform stream of one counter family (c0, c1, tag, n = 0, 1, ...).  batch > 1 computes that many counters ahead in one
    vectorised call, twice as many at every refill up to 1024 (the same values: the stream is a function of the counter alone) -- for
    the long streams of background chunks."""

    def __init__(self, c0, c1, tag, seed, batch=1):
        self.c0, self.c1, self.tag, self.seed, self.n, self.buf = int(c0), int(c1), int(tag), int(seed), 0, []
        self.batch = int(batch)
        self.flag = False

    def next(self):
        if not self.buf:
            if self.batch > 1:
                n = np.arange(self.n, self.n + self.batch, dtype=np.uint64)
                u0, u1 = uniforms_from_words(philox4x32(self.c0, self.c1, self.tag, n, self.seed))
                self.n += self.batch
                self.batch = min(2 * self.batch, 1024)
                self.buf = np.stack([u0, u1], axis=1).ravel()[::-1].tolist()
            else:
                w = philox_scalar((self.c0, self.c1, self.tag, self.n), (self.seed & M32, (self.seed >> 32) & M32))
                self.n += 1
                u0, u1 = uniforms_from_words([np.uint64(x) for x in w])
                self.buf = [float(u1), float(u0)]
        return self.buf.pop()

    def near(self, x, y, scale=None):
        s = max(abs(x), abs(y)) if scale is None else scale
        if abs(x - y) <= TOL * s:
            self.flag = True


def lfact(k):
    if k < 17:
        p = 1.0
        for i in range(2, k + 1):
            p = p * float(i)
        return math.log(p)
    x = float(k + 1)
    x2 = x * x
    return (x - 0.5) * math.log(x) - x + 0.91893853320467274178 + 1.0 / (12.0 * x) - 1.0 / (360.0 * x * x2) + 1.0 / (1260.0 * x * x2 * x2)


def _inversion(st, lam, t, p):
    F, k = p, 0
    while t > F and k < KMAX:
        st.near(t, F)
        k += 1
        p = p * lam / float(k)
        F = F + p
    st.near(t, F)
    return k


def poisson(lam, st):
    if not lam > 0.0:
        return 0
    if lam < PTRS_MIN:
        u = st.next()
        return _inversion(st, lam, u, math.exp(-lam))
    slam, loglam = math.sqrt(lam), math.log(lam)
    b = 0.931 + 2.53 * slam
    a = -0.059 + 0.02483 * b
    invalpha = 1.1239 + 1.1328 / (b - 3.4)
    vr = 0.9277 - 3.6224 / (b - 2.0)
    for _ in range(TRIES):
        U = st.next() - 0.5
        V = st.next()
        us = 0.5 - abs(U)
        kf = math.floor((2.0 * a / us + b) * U + lam + 0.43)
        if us >= 0.07 and V <= vr:
            return int(kf)
        if kf < 0.0 or (us < 0.013 and V > us):
            continue
        lhs = math.log(V) + math.log(invalpha) - math.log(a / (us * us) + b)
        rhs = -lam + kf * loglam - lfact(int(kf))
        st.near(lhs, rhs, max(1.0, abs(rhs)))
        if lhs <= rhs:
            return int(kf)
    return int(math.floor(lam + 0.5))


def ztp(lam, st):
    if lam < PTRS_MIN:
        u = st.next()
        p0 = math.exp(-lam)
        t = p0 + u * (1.0 - p0)
        return max(1, _inversion(st, lam, t, p0))
    for _ in range(TRIES):
        k = poisson(lam, st)
        if k > 0:
            return k
    return 1


def sub_records(sub_id, sub_len_kb, sub_accu, state):
    """Per sub-fragment (centre kb float32, contig label or -1 if inactive, RF count, contig length bp if circular else -1) --
    simulate.h: k_sim_prep.  The centres walk each bin in its orientation (SparseScorer.centres)."""
    sub_id = np.asarray(sub_id, dtype=np.int64).reshape(-1, 4)
    n_bins = len(sub_id)
    n_sub = sub_id[:, 3]
    sub_len = np.asarray(sub_len_kb, dtype=np.float32).reshape(-1, 3)
    accu = np.asarray(sub_accu, dtype=np.int64).reshape(-1, 3)
    S = int(n_sub.sum())
    start = (np.asarray(state["start_bp"]).astype(np.float32) / f32(1000.0)).astype(np.float32)
    fwd = np.asarray(state["ori"]) == 1
    centre = np.zeros(S, np.float32)
    label = np.zeros(S, np.int64)
    acc = np.zeros(S, np.int64)
    lbp = np.zeros(S, np.int64)
    for f in range(n_bins):
        lim = int(n_sub[f]) - 1
        run = start[f]
        for w in range(lim + 1):
            slot = w if fwd[f] else lim - w
            ln = sub_len[f, slot]
            i = sub_id[f, slot]
            centre[i] = f32(run + ln / f32(2.0))
            run = f32(run + ln)
            label[i] = int(state["id_c"][f]) if int(state["activ"][f]) == 1 else -1
            acc[i] = accu[f, slot]
            lbp[i] = int(state["l_cont_bp"][f]) if int(state["circ"][f]) == 1 else -1
    return centre, label, acc, lbp


def pair_lambda(rec, a, b, nfpb, param):
    """lambda(a, b) as the full likelihood prices the sub-pixel (float32, then 0 if negative): arrays a, b."""
    centre, label, acc, lbp = rec
    param = np.asarray(param, dtype=np.float32)
    norm = ((acc[a] * acc[b]).astype(np.float32) / f32(nfpb)).astype(np.float32)
    cis = label[a] == label[b]
    s = np.abs(centre[b] - centre[a]).astype(np.float32)
    r = rippe_f32(np.where(cis, s, f32(0)), param)
    circ = cis & (lbp[a] >= 0)
    if np.any(circ):
        s_tot = (np.where(circ, lbp[a], 1000).astype(np.float32) / f32(1000.0)).astype(np.float32)
        r = np.where(circ, rippe_circ_f32(np.where(circ, s, f32(0)), s_tot, param), r)
    lam = np.where(cis, (r * norm).astype(np.float32), (param[7] * norm).astype(np.float32)).astype(np.float32)
    lam = np.where((label[a] < 0) | (label[b] < 0), f32(0), lam)
    return np.maximum(lam, f32(0)).astype(np.float64)


def simulate(sub_id, sub_len_kb, sub_accu, nfpb, param, state, seed, rows=None):
    """-> (row, col, count, flagged_pairs, flagged_chunks): the list graal_simulate_contacts returns, and the draws that may differ
    from the GPU's by a last-place rounding (window pairs (a, b); background chunks (a, k)).
    rows: restate these rows only (rows are independent: the counters are (a, b, 0, .) and (a, k, 1, .)) -- the same five values,
    restricted to them.  For layouts whose dense rows make the loop over every row too slow."""
    param = np.asarray(param, dtype=np.float32).reshape(8)
    rec = sub_records(sub_id, sub_len_kb, sub_accu, state)
    centre, label, acc, lbp = rec
    S = len(centre)
    d_max = param[5]
    amax = int(acc.max()) if S else 1
    amax = max(amax, 1)
    out = {}
    flagged_pairs, flagged_chunks = set(), set()
    todo = range(S) if rows is None else sorted({int(a) for a in rows})
    assert all(0 <= a < S for a in todo)
    # window pairs, vectorised over each row's columns: the first uniform decides most of them (count 0)
    for a in todo:
        if label[a] < 0:
            continue
        b = np.arange(a + 1, S)
        w = b[(label[b] == label[a]) & (np.abs(centre[b] - centre[a]).astype(np.float32) < d_max)]
        if len(w) == 0:
            continue
        lam = pair_lambda(rec, np.full(len(w), a), w, nfpb, param)
        u0, _ = uniforms_from_words(philox4x32(a, w, 0, 0, seed))
        p0 = np.exp(-lam)
        small = lam < PTRS_MIN
        zero = (lam <= 0) | (small & (u0 <= p0))
        near0 = small & (lam > 0) & (np.abs(u0 - p0) <= TOL * np.maximum(u0, p0))
        for bb in w[near0]:
            flagged_pairs.add((a, int(bb)))
        for j in np.nonzero(~zero)[0]:
            st = Stream(a, w[j], 0, seed)
            c = poisson(float(lam[j]), st)
            if st.flag:
                flagged_pairs.add((a, int(w[j])))
            if c > 0:
                out[(a, int(w[j]))] = c
    # background chunks
    v_inter = param[7]
    for a in todo:
        if label[a] < 0:
            continue
        lmax_f = f32(v_inter * f32(f32(acc[a] * amax) / f32(nfpb)))
        if not lmax_f > 0:
            continue
        lmax = float(lmax_f)
        pm = 1.0 - math.exp(-lmax)
        for k in range((a + 1) // CHUNK, (S - 1) // CHUNK + 1):
            c_begin, c_end = max(a + 1, k * CHUNK), min(S, (k + 1) * CHUNK)
            st = Stream(a, k, 1, seed, batch=16)
            j = c_begin - 1
            while True:
                g = -math.log(st.next()) / lmax
                # (lambda_max is the same float32 on both sides and log's error is ~1e-16 relative: a skip can only tip within a few
                # 1e-16 g of an integer >= 1; flag 1e-9 g.  Not at 0: g > 0, floor(g) = 0 holds on both sides)
                if round(g) >= 1:
                    st.near(g, round(g), SKIP_TOL / TOL * max(1.0, g))
                st.near(g, float(c_end - j - 1), SKIP_TOL / TOL * max(1.0, g))
                if not g < float(c_end - j - 1):
                    break
                j = j + 1 + int(math.floor(g))
                if label[j] < 0:
                    continue
                if label[j] == label[a] and abs(f32(centre[j] - centre[a])) < d_max:
                    continue
                lb = float(f32(v_inter * f32(f32(acc[a] * acc[j]) / f32(nfpb))))
                v = st.next()
                qb = 1.0 - math.exp(-lb)
                st.near(v * pm, qb)
                if v * pm < qb:
                    out[(a, j)] = ztp(lb, st)
            if st.flag:
                flagged_chunks.add((a, k))
    keys = sorted(out)
    row = np.array([k[0] for k in keys], dtype=np.int32)
    col = np.array([k[1] for k in keys], dtype=np.int32)
    cnt = np.array([out[k] for k in keys], dtype=np.int32)
    return row, col, cnt, flagged_pairs, flagged_chunks


def brute_force_background(rec, a, c_begin, c_end, nfpb, param, rng):
    """Per-pair draw of a background range (numpy's Poisson): the distribution the skip sampler must reproduce."""
    centre, label, acc, lbp = rec
    param = np.asarray(param, dtype=np.float32)
    b = np.arange(c_begin, c_end)
    bg = (label[b] >= 0) & ~((label[b] == label[a]) & (np.abs(centre[b] - centre[a]).astype(np.float32) < param[5]))
    lam = np.where(bg, (param[7] * ((acc[a] * acc[b]).astype(np.float32) / f32(nfpb)).astype(np.float32)).astype(np.float32), 0)
    return b, rng.poisson(np.maximum(lam, 0).astype(np.float64))


def expected_lambda_matrix(sub_id, sub_len_kb, sub_accu, nfpb, param, state):
    """lambda of every pair a < b as two index arrays and the values (small layouts only)."""
    rec = sub_records(sub_id, sub_len_kb, sub_accu, state)
    S = len(rec[0])
    a, b = np.triu_indices(S, 1)
    return a, b, pair_lambda(rec, a, b, nfpb, np.asarray(param, dtype=np.float32))


def compare(got, want, flagged_pairs, flagged_chunks):
    """(entries that differ, entries that differ outside the flagged draws).  got / want = (row, col, count)."""
    g = {(int(r), int(c)): int(v) for r, c, v in zip(*got)}
    w = {(int(r), int(c)): int(v) for r, c, v in zip(*want)}
    diff = [k for k in set(g) | set(w) if g.get(k) != w.get(k)]
    unexplained = [k for k in diff if k not in flagged_pairs and (k[0], k[1] // CHUNK) not in flagged_chunks]
    return diff, unexplained
