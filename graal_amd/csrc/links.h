// links.h -- the likelihood every join between two contig ends would add, for every pair of ends the contacts support (graal_end_links).
// Included by graal_hip.hip after rings.h (it uses Ctx, Stat, centre_kb, rippe, to_q, jn_trans, model_math.h, score_common.h's
// score_entry, score_exit, STEP_CK, stream_blocks and CandTable, layout_slots.h's LayoutSlots and slot_claim, and wave_runs.h's run_sums).
// LayoutRecs, below, is shared with insert.h, span_moves.h and excise.h.
//
// Ends.  end = 2 * f + side of a LINEAR contig: side 0 its head (position 0), side 1 its tail (position l_cont - 1), f the fragment there.
// For ends eA < eB of different contigs A, B the joined layout is canonical: A oriented so that eA is its tail (A reversed iff eA is a head),
// B after it oriented so that eB is its head (B reversed iff eB is a tail); positions, start_bp and ori as m_paste writes them, the centres
// through centre_kb from the integer offsets.  L(eA, eB) = logL(joined) - logL(current) in the exact arithmetic, with the junction call's
// roundings: pairs inside A and inside B count as unchanged; every sub-fragment pair of A x B moves from its current trans price to its
// price in the joined layout (a contact: ob * (ln ex_new - ln ex_trans), rounded to Q once; a fragment pair's mass: -(sum of ex_new -
// ex_trans), rounded to Q once).  Under GRAAL_MODE_REF_TRANS_ACCU with bins of mixed RF counts two more terms belong to L:
//   - A x B pairs beyond the window that involve such a bin (v_inter * plain norm after the join, v_inter * indexed norm now);
//   - the MIRROR term: a reversed contig flips the orientation of its mixed bins, and the trans-branch indexing prices a pair by the
//     orientation of its lower-id bin: every pair (x of the reversed contig, mixed; y outside it, y > x) changes its trans price.
//     mirror[C] (one per contig, for its reversal) is summed once; a link adds it for each contig it reverses and takes off the part that
//     falls on the partner contig, whose pairs it prices directly.
//
// Which links are listed: the pairs of ends with at least one contact between their contigs inside the window (sub-fragment centre
// distance < d_max) in the joined orientation.  Kernels, all on the engine's stream:
//   slots_count (k_jn_count / scan) / k_ln_prep -- slots (layout_slots.h's numbering), a 48-byte
//                 record per slot, a 32-byte record per sub-fragment and a 32-byte record per contig label (end fragments, bp length,
//                 eligibility: linear with >= min_frags fragments);
//   k_ln_nnz<COUNT> -- streams the row-sorted COO list, 64 contacts per wave; for a contact between two eligible contigs each of the 4
//                 end combinations yields a record when its joined distance is inside the window or its term is not zero (the quirk).
//                 Records are summed per run of equal keys inside the wave (segmented shuffle scans) and only a run's last lane touches
//                 the table: the count pass counts those lanes (an upper bound of the distinct keys that sizes the table), the insert
//                 pass adds into an open-addressing table keyed by (eA << 32 | eB) with 64-bit CAS and linear probing;
//   k_ln_flag, hipCUB DeviceSelect::Flagged, k_ln_keys, a radix sort by key, k_ln_gather -- the listed keys in (end_a, end_b) order;
//   k_ln_mass  -- a wave per (link, group of 8 fragments of A walked from eA); lanes are 8 x 8 fragment pairs, the tile steps along B from
//                 eB and the wave stops when every pair has left the window (the joined gap only grows along both walks);
//   k_ln_mirror, k_ln_quirk -- only with GRAAL_MODE_REF_TRANS_ACCU and mixed bins: mirror[C] (one block per mixed bin, all later bins),
//                 and the A x B pairs with a mixed bin (beyond the window, and the mirror's part on the partner): a wave per (link, group
//                 of 8 fragments of A) as k_ln_mass, over all of B -- the only work that grows with contig length outside the window;
//   k_ln_out   -- q = direct + mirrors of the reversed contigs, and a status byte.
// What a contact contributes per end combination is formed by the contact unit (ln_contact, ln_comb, ln_mirror_term, ln_comb_term),
// which takes the count as an argument: links_boot.h's k_lkb_nnz calls it with a replicate's count.  ln_links is graal_end_links between
// score_entry and score_exit; graal_end_links_bootstrap (links_boot.h) runs it too.
#pragma once

namespace {

constexpr unsigned long long LN_EMPTY = ~0ull;

struct LnSub { int label, frag, meta, acc, start, len, lbp, pad; };   // meta: sub k | n << 2 | fwd << 4 | mixed << 5 | eligible << 6 | circ << 7
                                                                    // acc: RF count | RF count of the bin's last sub-fragment << 16
struct LnFrag { int frag, start, len, fwd; Stat st; };              // per slot
struct LnCtg { int head, tail, first, cnt, lbp, elig, nmix, pad; };   // per contig label; nmix: its bins of mixed RF counts


__global__ __launch_bounds__(256) void k_ln_prep(SoaPtr s, int n, int min_frags, const Stat* __restrict__ stat, const int* __restrict__ sub_ids,
                                                 const int* __restrict__ cnt, const int* __restrict__ base, int* __restrict__ slot_of,
                                                 int* __restrict__ lab, LnFrag* __restrict__ fr, LnSub* __restrict__ sub, LnCtg* __restrict__ ctg,
                                                 unsigned long long* __restrict__ n_elig, unsigned* __restrict__ err)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int slot = slot_claim(s, n, f, cnt, base, slot_of, err);
    if (slot < 0) { lab[f] = -1; return; }
    const int c = s.p[F_IDC][f], pos = s.p[F_POS][f];
    lab[f] = c;
    const Stat st = stat[f];
    const bool fwd = s.p[F_ORI][f] == 1, circ = s.p[F_CIRC][f] == 1;
    const int start = s.p[F_START][f], len = s.p[F_LEN][f], lbp = s.p[F_LCONTBP][f];
    const bool elig = !circ && cnt[c] >= min_frags;
    LnFrag r;
    r.frag = f; r.start = start; r.len = len; r.fwd = fwd ? 1 : 0; r.st = st;
    fr[slot] = r;
    if (pos == 0) {
        ctg[c].head = f; ctg[c].first = base[c]; ctg[c].cnt = cnt[c]; ctg[c].lbp = lbp; ctg[c].elig = elig ? 1 : 0;
        if (elig) atomicAdd(n_elig, 1ull);
    }
    if (pos == cnt[c] - 1) ctg[c].tail = f;
    const int last = stat_accu(st, st.n - 1);
    const int mixed = stat_uniform(st) ? 0 : 1;
    if (mixed && elig) atomicAdd(&ctg[c].nmix, 1);
    int4 ids = make_int4(f, 0, 0, 1);
    if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[f];
    for (int k = 0; k < st.n; k++) {
        LnSub u;
        u.label = c; u.frag = f; u.start = start; u.len = len; u.lbp = lbp; u.pad = 0;
        u.meta = k | (st.n << 2) | ((fwd ? 1 : 0) << 4) | (mixed << 5) | ((elig ? 1 : 0) << 6) | ((circ ? 1 : 0) << 7);
        u.acc = stat_accu(st, k) | (last << 16);                     // (RF counts are <= 30000)
        sub[sel3(ids.x, ids.y, ids.z, k)] = u;
    }
}

// The slots and records of a layout (slots_count / k_ln_prep) and what is summed per contig label.  links.h, insert.h and span_moves.h
// each own one instance: no state is shared between their calls.
struct LayoutRecs {
    int n = 0, S = 0;
    LayoutSlots L;
    DevBuf<int> lab;
    DevBuf<LnFrag> fr;
    DevBuf<LnSub> sub;
    DevBuf<LnCtg> ctg;
    DevBuf<long long> mir; DevBuf<int> mirbad;
    DevBuf<unsigned long long> ctr;      // [0] records counted, [1] listed keys, [2] eligible contigs, [3] insert.h's pair records
};

// Sized to the engine's (n, S), reallocated when they change.
int recs_reserve(Ctx* h, LayoutRecs& R)
{
    const int n = h->n, S = h->n_sub_total;
    if (R.n == n && R.S == S) return GRAAL_OK;
    if (const int rc = slots_reserve(h, R.L)) return rc;
    CK(group_realloc(R.n, n, R.lab, n, R.fr, n, R.sub, std::max(S, 1), R.ctg, n + 3, R.mir, n + 3, R.mirbad, n + 3, R.ctr, 4));
    R.S = S;
    return GRAAL_OK;
}

// The records of the current layout, on the engine's stream.  R.L.err collects the flags of a corrupt layout: the caller reads it back
// (slots_read_err) before anything trusts the slots or the sub-fragment records.
int recs_build(Ctx* h, LayoutRecs& R, int min_frags)
{
    const int n = R.n;
    hipStream_t s = h->stream;
    int rc = GRAAL_OK;
    do {
        STEP_CK(hipMemsetAsync(R.ctr, 0, sizeof(unsigned long long) * 4, s));
        STEP_CK(hipMemsetAsync(R.ctg, 0, sizeof(LnCtg) * (size_t)(n + 3), s));   // (labels no fragment holds: not eligible)
        STEP_CK(hipMemsetAsync(R.fr, 0, sizeof(LnFrag) * (size_t)n, s));
        STEP_CK(hipMemsetAsync(R.mir, 0, sizeof(long long) * (size_t)(n + 3), s));
        STEP_CK(hipMemsetAsync(R.mirbad, 0, sizeof(int) * (size_t)(n + 3), s));
        if ((rc = slots_count(h, R.L))) break;
        k_ln_prep<<<blocks_for(n, 256), 256, 0, s>>>(h->soa[h->cur], n, min_frags, h->stat_frag, h->d_sub_ids, R.L.cnt, R.L.base, R.L.slot, R.lab,
                                                     R.fr, R.sub, R.ctg, &R.ctr[2], R.L.err);
        STEP_CK(hipGetLastError());
    } while (false);
    return rc;
}

struct LnBuf {
    LayoutRecs R;
    CandTable T;
    // the table (T) and the per-link arrays grow to the largest size a call needed (within GRAAL_LINKS_MAX_BYTES)
    DevBuf<unsigned long long> ko, ks; DevBuf<int> vo, vs;
    DevBuf<long long> q, c, ch, choff; DevBuf<int> bad; DevBuf<unsigned char> st;
    DevBuf<int> ea, eb;
    size_t lcap = 0;
    long long n_links = -1;                                          // -1: no result to fetch
    // graal_end_links_best: per end (2n) the best Q and partner, the mutual flag, and the mutual links compacted
    DevBuf<long long> bq; DevBuf<int> be; DevBuf<unsigned char> bflag; DevBuf<int> bsel, mea, meb;
    DevBuf<long long> mq; size_t bcap = 0;
    long long n_mutual = -1;                                         // -1: no result to fetch
    // graal_end_links_bootstrap (links_boot.h).  Per table slot the link's index (-1: not listed); per contig label the contact part of
    // mirror[C] under the data's counts (kc_mir) and a flag for a replicate term of it that does not fit Q (kc_bad); per link the fixed
    // part M, the statistics, a flag for an unrepresentable replicate term and the call's status; per batch of replicates the contact
    // sums C[r * m + link] (then L*_r in place), mirc[r * (n + 3) + label] and the per-end best Q / partner [r * 2n + end].
    DevBuf<int> k_s2l; DevBuf<long long> kc_mir; DevBuf<int> kc_bad;
    DevBuf<long long> k_fix, k_sum, k_mn, k_mx; DevBuf<int> k_sup, k_mut, k_lbad; DevBuf<unsigned char> k_st; size_t kcap = 0;
    DevBuf<long long> kb_c, kb_mir, kb_bq; DevBuf<int> kb_be;
    std::vector<long long> k_rep;                                    // the replicate matrix of the last call that wanted it (host)
    long long boot_links = -1;                                       // -1: no result to fetch
    int boot_rep = 0; bool boot_want = false;
};

void ln_free(LnBuf* b) { delete b; }

__device__ __forceinline__ int ln_k(int meta) { return meta & 3; }
__device__ __forceinline__ bool ln_fwd(int meta) { return (meta >> 4) & 1; }
__device__ __forceinline__ bool ln_mixed(int meta) { return (meta >> 5) & 1; }
__device__ __forceinline__ bool ln_elig(int meta) { return (meta >> 6) & 1; }

// start_bp in the joined layout of a fragment (start, len) of a contig of lbp bp: first (A) or second (B) in the join, reversed or not
__device__ __forceinline__ int ln_new_start(int start, int len, int lbp, int lbp_first, bool first, bool rev)
{
    const int s = rev ? lbp - start - len : start;
    return first ? s : lbp_first + s;
}

// 64-bit key mixer (splitmix64's finaliser) and the table slot of `key`: linear probing from the mixed key, claimed with a 64-bit CAS
__device__ __forceinline__ unsigned long long ln_mix(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ long long ln_slot(unsigned long long* __restrict__ keys, unsigned long long cap, unsigned long long key,
                                             unsigned* __restrict__ err)
{
    unsigned long long i = __umul64hi(ln_mix(key), cap);
    for (unsigned long long t = 0; t < cap; t++) {
        const unsigned long long old = atomicCAS(&keys[i], LN_EMPTY, key);
        if (old == LN_EMPTY || old == key) return (long long)i;
        if (++i == cap) i = 0;
    }
    atomicOr(err, 4u);                                               // (cannot happen: the table holds more slots than records)
    return -1;
}

// The find-only probe of the same table: the slot that holds `key`, or -1 (links_boot.h: a replicate never inserts).
__device__ __forceinline__ long long ln_find(const unsigned long long* __restrict__ keys, unsigned long long cap, unsigned long long key)
{
    unsigned long long i = __umul64hi(ln_mix(key), cap);
    for (unsigned long long t = 0; t < cap; t++) {
        const unsigned long long old = keys[i];
        if (old == key) return (long long)i;
        if (old == LN_EMPTY) return -1;
        if (++i == cap) i = 0;
    }
    return -1;
}

// ---- The contact unit: what a contact (X, Y) contributes per end combination, with the count left out.  k_ln_nnz multiplies by the
// data's count, links_boot.h's k_lkb_nnz by a replicate's: both round count * unit to Q once, so a replicate that draws the count itself
// gives k_ln_nnz's words.
// Per contact: pair (both contigs eligible: the contact yields link records), mq (the mirror's contact part: the lower-id bin is mixed
// and its contig eligible), the RF-count products in the plain indexing (prod) and in the current trans indexing (prod_t), and the
// mirror's unit m_t = ln ex_trans(lower bin flipped) - ln ex_trans(now), used when m_on.
struct LnContact { bool pair, mq, x_low, m_on; int prod, prod_t, mlabel; double m_t; };

__device__ __forceinline__ void ln_contact(const LnSub& X, const LnSub& Y, int quirk, float nfpb, const Par& par, LnContact& U)
{
    const bool diff = X.label != Y.label;                            // (lanes past the list hold label -1 twice: no contact)
    U.pair = diff && ln_elig(X.meta) && ln_elig(Y.meta);
    // the quirk: the lower-id bin's orientation picks the trans price's indexing
    U.x_low = X.frag < Y.frag;
    const LnSub& lo = U.x_low ? X : Y;
    U.mq = quirk && diff && ln_mixed(lo.meta) && ln_elig(lo.meta);
    U.mlabel = lo.label;
    const int own_x = X.acc & 0xffff, own_y = Y.acc & 0xffff;
    U.prod = own_x * own_y;
    U.prod_t = U.prod;
    int prod_f = U.prod;                                             // the current trans indexing, and with the lower bin flipped
    if (quirk && diff) {
        const int own_l = lo.acc & 0xffff, last_l = lo.acc >> 16, other = U.x_low ? own_y : own_x;
        U.prod_t = (ln_fwd(lo.meta) ? own_l : last_l) * other;
        prod_f = (ln_fwd(lo.meta) ? last_l : own_l) * other;
    }
    U.m_on = U.mq && prod_f != U.prod_t;
    U.m_t = 0.0;
    if (U.m_on) {
        const float et = par.v_inter * ((float)U.prod_t / nfpb), ef = par.v_inter * ((float)prod_f / nfpb);
        U.m_t = mm_ln(ef) - mm_ln(et);
    }
}

// the mirror's contact term of a contact that counts ob
__device__ __forceinline__ void ln_mirror_term(const LnContact& U, double ob, long long& m_term, bool& m_bad)
{
    m_term = 0; m_bad = false;
    if (U.m_on) {
        m_term = to_q(ob * U.m_t);
        if (m_term == Q_BAD) { m_bad = true; m_term = 0; }
    }
}

// ln of the contact's current trans price
__device__ __forceinline__ double ln_contact_trans(const LnContact& U, float nfpb, const Par& par)
{
    return mm_ln(par.v_inter * ((float)U.prod_t / nfpb));
}

// Per (contact of a pair, end combination c = side of X's contig << 1 | side of Y's): the link's key, whether the joined distance is
// inside the window, the unit t = ln ex_joined - ln ex_trans (has_t: it is not exactly 0), and whether the mirror's contact term comes
// off (the lower bin's contig is reversed by this link).
struct LnComb { unsigned long long key; double t; bool has_t, in_win, sub_m; };

__device__ __forceinline__ void ln_comb(const LnContact& U, const LnSub& X, const LnSub& Y, const LnCtg& CX, const LnCtg& CY, const Stat& SX,
                                        const Stat& SY, int c, double ln_et, float nfpb, const Par& par, LnComb& G)
{
    const int sx = c >> 1, sy = c & 1;
    const int ex = 2 * (sx ? CX.tail : CX.head) + sx, ey = 2 * (sy ? CY.tail : CY.head) + sy;
    const bool x_first = ex < ey;
    // A (first) is reversed iff its end is a head; B (second) iff its end is a tail
    const bool rev_x = x_first ? sx == 0 : sx == 1, rev_y = x_first ? sy == 1 : sy == 0;
    const int lbp_first = x_first ? X.lbp : Y.lbp;
    const int nsx = ln_new_start(X.start, X.len, X.lbp, lbp_first, x_first, rev_x);
    const int nsy = ln_new_start(Y.start, Y.len, Y.lbp, lbp_first, !x_first, rev_y);
    const float cx = centre_kb(nsx, ln_fwd(X.meta) != rev_x, SX, ln_k(X.meta));
    const float cy = centre_kb(nsy, ln_fwd(Y.meta) != rev_y, SY, ln_k(Y.meta));
    const float sd = fabsf(cy - cx);
    G.in_win = sd < par.d_max;
    G.t = 0.0;
    // (at |d| >= d_max rippe is v_inter exactly: the joined and the trans prices are the same float32 value unless the indexing differs)
    G.has_t = !(sd >= par.d_max && U.prod_t == U.prod && par.v_inter >= 0.0f);
    if (G.has_t) {
        const float exn = rippe(sd, par) * ((float)U.prod / nfpb);
        G.t = mm_ln(exn) - ln_et;
    }
    G.sub_m = U.mq && (U.x_low ? rev_x : rev_y);                     // the mirror's part on the partner: priced above
    G.key = x_first ? ((unsigned long long)ex << 32) | (unsigned)ey : ((unsigned long long)ey << 32) | (unsigned)ex;
}

// the record term of a combination for a contact that counts ob (m_term, m_bad: ln_mirror_term's for the same count)
__device__ __forceinline__ void ln_comb_term(const LnComb& G, double ob, long long m_term, bool m_bad, long long& q, bool& bad)
{
    q = 0; bad = false;
    if (G.has_t) {
        const long long t = to_q(ob * G.t);
        if (t == Q_BAD) bad = true; else q = t;
    }
    if (G.sub_m) { q -= m_term; bad = bad || m_bad; }
}

// The contact pass.  COUNT: count the records a wave would insert (after its run sums).  Otherwise insert them, and sum the contact part
// of mirror[C] (the quirk) per contig.
template <bool COUNT>
__global__ __launch_bounds__(256) void k_ln_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt, long long nnz,
                                                const LnSub* __restrict__ sub, const Stat* __restrict__ stat, const LnCtg* __restrict__ ctg,
                                                float nfpb, Par par, int quirk, unsigned long long cap, unsigned long long* __restrict__ keys,
                                                long long* __restrict__ tq, long long* __restrict__ tc, int* __restrict__ tf,
                                                long long* __restrict__ mir, int* __restrict__ mirbad, unsigned long long* __restrict__ n_rec,
                                                unsigned* __restrict__ err)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    unsigned long long n_wave = 0;                                   // COUNT: the wave's records, one atomic at the end
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {   // (wave-uniform bounds: the run sums need the whole wave)
        const long long k = k0 + lane;
        LnSub X = {-1, -1, 0, 0, 0, 0, 0, 0}, Y = X;                   // (lanes past the list: no contig, no bin, no flags)
        if (k < nnz) { X = sub[row[k]]; Y = sub[col[k]]; }
        LnContact U;
        ln_contact(X, Y, quirk, nfpb, par, U);
        const bool pair = U.pair, mq = U.mq;
        if (__ballot(pair || mq) == 0ull) continue;
        const double ob = k < nnz ? (double)__int_as_float(cnt[k]) : 0.0;
        long long m_term;
        bool m_bad;
        ln_mirror_term(U, ob, m_term, m_bad);
        if (!COUNT) {                                                // mirror[C]'s contacts, summed per run of the lower bin's contig
            const unsigned long long mk = (mq && (m_term != 0 || m_bad)) ? (unsigned long long)U.mlabel : LN_EMPTY;
            if (__ballot(mk != LN_EMPTY) != 0ull) {
                long long v0 = m_term, v1 = m_bad ? 1 : 0, v2 = 0;
                bool tail;
                run_sums(mk, tail, v0, v1, v2);
                if (tail && mk != LN_EMPTY) {
                    if (v0 != 0) atomicAdd((unsigned long long*)&mir[mk], (unsigned long long)v0);
                    if (v1 != 0) atomicAdd(&mirbad[mk], (int)v1);
                }
            }
        }
        if (__ballot(pair) == 0ull) continue;
        LnCtg CX, CY;
        Stat SX, SY;
        if (pair) { CX = ctg[X.label]; CY = ctg[Y.label]; SX = stat[X.frag]; SY = stat[Y.frag]; }
        const double ln_et = ln_contact_trans(U, nfpb, par);
#pragma unroll 1
        for (int c = 0; c < 4; c++) {
            unsigned long long key = LN_EMPTY;
            long long q = 0, n_in = 0, fl = 0;
            if (pair) {
                LnComb G;
                ln_comb(U, X, Y, CX, CY, SX, SY, c, ln_et, nfpb, par, G);
                bool bad;
                ln_comb_term(G, ob, m_term, m_bad, q, bad);
                if (G.in_win || q != 0 || bad) {
                    key = G.key;
                    n_in = G.in_win ? (long long)llrint(ob) : 0;
                    fl = (bad ? 1 : 0) + (G.in_win ? (1ll << 32) : 0);
                }
            }
            if (__ballot(key != LN_EMPTY) == 0ull) continue;
            bool tail;
            run_sums(key, tail, q, n_in, fl);
            const bool rec = tail && key != LN_EMPTY;
            if (COUNT) {
                n_wave += (unsigned long long)__popcll(__ballot(rec));
            } else if (rec) {
                const long long i = ln_slot(keys, cap, key, err);
                if (i >= 0) {
                    if (q != 0) atomicAdd((unsigned long long*)&tq[i], (unsigned long long)q);
                    if (n_in != 0) atomicAdd((unsigned long long*)&tc[i], (unsigned long long)n_in);
                    const int b = ((fl & 0xffffffffll) ? 1 : 0) | ((fl >> 32) ? 2 : 0);
                    if (b) atomicOr(&tf[i], b);
                }
            }
        }
    }
    if (COUNT && lane == 0 && n_wave) atomicAdd(n_rec, n_wave);     // (a single counter: one atomic per wave, not per contact group)
}

// the listed slots of the table (a contact inside the window), for hipCUB's DeviceSelect::Flagged; then the keys of the selected slots
__global__ void k_ln_flag(const unsigned long long* __restrict__ keys, const int* __restrict__ tf, long long cap, unsigned char* __restrict__ sel)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) sel[i] = (keys[i] != LN_EMPTY && (tf[i] & 2)) ? 1 : 0;
}

__global__ void k_ln_keys(long long m, const unsigned long long* __restrict__ keys, const int* __restrict__ vo, unsigned long long* __restrict__ ko)
{
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < m) ko[j] = keys[vo[j]];
}

__global__ void k_ln_gather(long long m, const unsigned long long* __restrict__ ks, const int* __restrict__ vs, const long long* __restrict__ tq,
                            const long long* __restrict__ tc, const int* __restrict__ tf, const int* __restrict__ lab,
                            const LnCtg* __restrict__ ctg, long long* __restrict__ q, long long* __restrict__ c, int* __restrict__ bad,
                            long long* __restrict__ ch, int* __restrict__ ea, int* __restrict__ eb)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = vs[k];
    const unsigned long long key = ks[k];
    ea[k] = (int)(key >> 32); eb[k] = (int)(key & 0xffffffffull);
    q[k] = tq[i]; c[k] = tc[i]; bad[k] = tf[i] & 1;
    ch[k] = (ctg[lab[ea[k] >> 1]].cnt + 7) / 8;                      // k_ln_mass: groups of 8 fragments of A
}

// one side of a link: the contig's slots walked from the end, its bp length and its orientation in the join
struct LnSide { int first, cnt, lbp; bool from_tail, rev; };

__device__ __forceinline__ LnSide ln_side(const LnCtg& C, int side, bool is_first)
{
    LnSide s;
    s.first = C.first; s.cnt = C.cnt; s.lbp = C.lbp;
    s.from_tail = side == 1;                                         // the walk starts at the joined end
    s.rev = is_first ? side == 0 : side == 1;
    return s;
}
__device__ __forceinline__ int ln_walk(const LnSide& s, int i) { return s.from_tail ? s.first + s.cnt - 1 - i : s.first + i; }
__device__ __forceinline__ int ln_gap(const LnSide& s, const LnFrag& x) { return s.from_tail ? s.lbp - (x.start + x.len) : x.start; }

// mass term of fragment pair (x of A, y of B): sum over sub-fragment pairs of ex_joined - ex_trans (current orientation, `quirk` indexing)
__device__ __forceinline__ double ln_pair_mass(const LnFrag& x, int nsx, bool fx, const LnFrag& y, int nsy, bool fy, float nfpb, const Par& par,
                                               int quirk)
{
    double acc = 0.0;
    const int lx = stat_accu(x.st, x.st.n - 1), ly = stat_accu(y.st, y.st.n - 1);
    for (int a = 0; a < x.st.n; a++) {
        const float ca = centre_kb(nsx, fx, x.st, a);
        const int ax = stat_accu(x.st, a);
        for (int b = 0; b < y.st.n; b++) {
            const int ay = stat_accu(y.st, b);
            const float ex = rippe(fabsf(centre_kb(nsy, fy, y.st, b) - ca), par) * ((float)(ax * ay) / nfpb);
            acc += (double)ex - (double)jn_trans(ax, ay, lx, ly, x.fwd, y.fwd, x.frag, y.frag, nfpb, par, quirk);
        }
    }
    return acc;
}

__device__ __forceinline__ long long ln_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void ln_block_add(long long v, long long nb, long long* __restrict__ q, int* __restrict__ bad)
{
    v = ln_wave_sum(v);
    nb = ln_wave_sum(nb);
    if ((threadIdx.x & 63) == 0) {
        if (v != 0) atomicAdd((unsigned long long*)q, (unsigned long long)v);
        if (nb != 0) atomicAdd(bad, (int)nb);
    }
}

// the link of wave group W: the last k with choff[k] <= W (links with no group never match)
__device__ __forceinline__ long long ln_link_of_group(const long long* __restrict__ choff, long long m, long long W)
{
    long long lo = 0, hi = m - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if (choff[mid] <= W) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// A wave's lanes are 8 x 8 fragment pairs.  A lane's fragment of A in group g (8 fragments walked from eA), as the join places it; live
// while its own gap to the joined end is inside the window.
struct LnRow { LnFrag x; int gx, nsx; bool fx, live; };

__device__ __forceinline__ void ln_group_row(const LnSide& A, int g, const LnFrag* __restrict__ fr, int reach_bp, LnRow& r)
{
    const int i = g * 8 + ((threadIdx.x & 63) >> 3);
    r.gx = 0; r.nsx = 0; r.fx = false; r.live = i < A.cnt;
    if (r.live) {
        r.x = fr[ln_walk(A, i)];
        r.gx = ln_gap(A, r.x);
        r.nsx = ln_new_start(r.x.start, r.x.len, A.lbp, A.lbp, true, A.rev);
        r.fx = (r.x.fwd != 0) != A.rev;
        r.live = r.gx <= reach_bp;
    }
}

// The mass of a group's rows against the window of B: the tile steps along B from eB, a Q-rounded term per fragment pair.  k_ln_mass and
// k_lb_mass both price through here, so both give every fragment pair the same term.
__device__ __forceinline__ void ln_group_mass(const LnRow& r, const LnSide& A, const LnSide& B, const LnFrag* __restrict__ fr, float nfpb,
                                              const Par& par, int quirk, int reach_bp, long long& sum, long long& nb)
{
    const int jl = threadIdx.x & 7;
    for (int j0 = 0; ; j0 += 8) {
        const int j = j0 + jl;
        bool in = r.live && j < B.cnt;
        LnFrag y;
        int gy = 0;
        if (in) { y = fr[ln_walk(B, j)]; gy = ln_gap(B, y); in = (long long)r.gx + gy <= reach_bp; }
        if (__ballot(in) == 0ull) break;                             // (the gap grows along both walks: no later tile is in the window)
        if (in) {
            const int nsy = ln_new_start(y.start, y.len, B.lbp, A.lbp, false, B.rev);
            const long long t = to_q_fast(ln_pair_mass(r.x, r.nsx, r.fx, y, nsy, (y.fwd != 0) != B.rev, nfpb, par, quirk));
            if (t == Q_BAD) nb++; else sum -= t;
        }
    }
}

__global__ __launch_bounds__(256) void k_ln_mass(long long m, long long n_groups, const long long* __restrict__ choff, const long long* __restrict__ ch,
                                                 const int* __restrict__ ea, const int* __restrict__ eb, const int* __restrict__ lab,
                                                 const LnCtg* __restrict__ ctg, const LnFrag* __restrict__ fr, float nfpb, Par par, int quirk,
                                                 int reach_bp, long long* __restrict__ q, int* __restrict__ bad)
{
    const long long W = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (W >= n_groups) return;
    const long long k = ln_link_of_group(choff, m, W);
    const long long g = W - choff[k];
    if (g < 0 || g >= ch[k]) return;
    const int e_a = ea[k], e_b = eb[k];
    const LnCtg CA = ctg[lab[e_a >> 1]], CB = ctg[lab[e_b >> 1]];
    const LnSide A = ln_side(CA, e_a & 1, true), B = ln_side(CB, e_b & 1, false);
    LnRow r;
    ln_group_row(A, (int)g, fr, reach_bp, r);
    long long sum = 0, nb = 0;
    ln_group_mass(r, A, B, fr, nfpb, par, quirk, reach_bp, sum, nb);
    ln_block_add(sum, nb, &q[k], &bad[k]);
}

// mirror mass term of bins x (mixed, flipped) and y (x < y): -(sum of trans(x flipped) - trans(x as now)), rounded to Q
__device__ __forceinline__ long long ln_mirror_q(const LnFrag& x, const LnFrag& y, float nfpb, const Par& par)
{
    double acc = 0.0;
    const int lx = stat_accu(x.st, x.st.n - 1);
    for (int a = 0; a < x.st.n; a++) {
        const int ax = stat_accu(x.st, a);
        const int now = x.fwd ? ax : lx, flip = x.fwd ? lx : ax;
        for (int b = 0; b < y.st.n; b++) {
            const int ay = stat_accu(y.st, b);
            acc += (double)(par.v_inter * ((float)(flip * ay) / nfpb)) - (double)(par.v_inter * ((float)(now * ay) / nfpb));
        }
    }
    const long long q = to_q(acc);
    return q == Q_BAD ? Q_BAD : -q;
}

// mirror[C], the mass part: one block per mixed bin x of an eligible contig, against every later bin of another contig
__global__ __launch_bounds__(256) void k_ln_mirror(int n, const int* __restrict__ ubins, const int* __restrict__ slot_of, const int* __restrict__ lab,
                                                   const LnCtg* __restrict__ ctg, const LnFrag* __restrict__ fr, float nfpb, Par par,
                                                   long long* __restrict__ mir, int* __restrict__ mirbad)
{
    const int xf = ubins[blockIdx.x];
    if (xf < 0 || xf >= n || slot_of[xf] < 0) return;
    const int c = lab[xf];
    if (!ctg[c].elig) return;
    const LnFrag x = fr[slot_of[xf]];
    if (x.st.n < 1) return;
    long long sum = 0, nb = 0;
    for (int y = xf + 1 + (int)threadIdx.x; y < n; y += (int)blockDim.x) {
        if (lab[y] == c || slot_of[y] < 0) continue;
        const long long t = ln_mirror_q(x, fr[slot_of[y]], nfpb, par);
        if (t == Q_BAD) nb++; else sum += t;
    }
    ln_block_add(sum, nb, &mir[c], &mirbad[c]);
}

// per link, the A x B pairs with a mixed bin: beyond the window their joined price (v_inter * plain norm) differs from the indexed trans
// price; and the mirror of a reversed contig counted a pair (its mixed bin, the partner's later bin) that the link prices directly.
__device__ __forceinline__ void ln_quirk_pair(const LnFrag& x, const LnFrag& y, bool beyond, bool rev_x, bool rev_y, float nfpb, const Par& par,
                                              long long& sum, long long& nb)
{
    if (beyond) {
        double acc = 0.0;
        const int lx = stat_accu(x.st, x.st.n - 1), ly = stat_accu(y.st, y.st.n - 1);
        for (int a = 0; a < x.st.n; a++)
            for (int b = 0; b < y.st.n; b++) {
                const int ax = stat_accu(x.st, a), ay = stat_accu(y.st, b);
                acc += (double)(par.v_inter * ((float)(ax * ay) / nfpb)) - (double)jn_trans(ax, ay, lx, ly, x.fwd, y.fwd, x.frag, y.frag, nfpb, par, 1);
            }
        const long long t = to_q(acc);
        if (t == Q_BAD) nb++; else sum -= t;
    }
    if (rev_x && !stat_uniform(x.st) && x.frag < y.frag) {
        const long long t = ln_mirror_q(x, y, nfpb, par);
        if (t == Q_BAD) nb++; else sum -= t;
    }
    if (rev_y && !stat_uniform(y.st) && y.frag < x.frag) {
        const long long t = ln_mirror_q(y, x, nfpb, par);
        if (t == Q_BAD) nb++; else sum -= t;
    }
}

// Group g of 8 fragments of A over ALL of B: a pair is priced when one of its bins is mixed (ln_quirk_pair)
__device__ __forceinline__ void ln_group_quirk(const LnSide& A, const LnSide& B, int g, const LnFrag* __restrict__ fr, float nfpb, const Par& par,
                                               int reach_bp, long long& sum, long long& nb)
{
    const int lane = threadIdx.x & 63, i = g * 8 + (lane >> 3);
    if (i >= A.cnt) return;
    const LnFrag x = fr[ln_walk(A, i)];
    const int gx = ln_gap(A, x);
    const bool mx = !stat_uniform(x.st);
    for (int j = lane & 7; j < B.cnt; j += 8) {
        const LnFrag y = fr[ln_walk(B, j)];
        if (!mx && stat_uniform(y.st)) continue;
        ln_quirk_pair(x, y, (long long)gx + ln_gap(B, y) > reach_bp, A.rev, B.rev, nfpb, par, sum, nb);
    }
}

// A wave per (link, group of 8 fragments of A) -- k_ln_mass's groups -- over ALL of B.  Links whose two contigs hold no mixed bin return at
// once.
__global__ __launch_bounds__(256) void k_ln_quirk(long long m, long long n_groups, const long long* __restrict__ choff, const long long* __restrict__ ch,
                                                  const int* __restrict__ ea, const int* __restrict__ eb, const int* __restrict__ lab,
                                                  const LnCtg* __restrict__ ctg, const LnFrag* __restrict__ fr, float nfpb, Par par, int reach_bp,
                                                  long long* __restrict__ q, int* __restrict__ bad)
{
    const long long W = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (W >= n_groups) return;
    const long long k = ln_link_of_group(choff, m, W);
    const long long g = W - choff[k];
    if (g < 0 || g >= ch[k]) return;
    const int e_a = ea[k], e_b = eb[k];
    const LnCtg CA = ctg[lab[e_a >> 1]], CB = ctg[lab[e_b >> 1]];
    if (CA.nmix == 0 && CB.nmix == 0) return;
    const LnSide A = ln_side(CA, e_a & 1, true), B = ln_side(CB, e_b & 1, false);
    if (__ballot(g * 8 + ((threadIdx.x & 63) >> 3) < A.cnt) == 0ull) return;
    long long sum = 0, nb = 0;
    ln_group_quirk(A, B, (int)g, fr, nfpb, par, reach_bp, sum, nb);
    ln_block_add(sum, nb, &q[k], &bad[k]);
}

// the mirrors of the contigs a link (eA, eB) reverses: A when its end is a head, B when its end is a tail
__device__ __forceinline__ void ln_add_mirrors(int e_a, int e_b, const int* __restrict__ lab, const long long* __restrict__ mir,
                                               const int* __restrict__ mirbad, long long& v, int& b)
{
    const int ca = lab[e_a >> 1], cb = lab[e_b >> 1];
    if ((e_a & 1) == 0) { v += mir[ca]; b += mirbad[ca]; }
    if ((e_b & 1) == 1) { v += mir[cb]; b += mirbad[cb]; }
}

__global__ void k_ln_out(long long m, const int* __restrict__ ea, const int* __restrict__ eb, const int* __restrict__ lab,
                         const long long* __restrict__ mir, const int* __restrict__ mirbad, int quirk, long long* __restrict__ q,
                         const int* __restrict__ bad, unsigned char* __restrict__ st)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    long long v = q[k];
    int b = bad[k];
    if (quirk) ln_add_mirrors(ea[k], eb[k], lab, mir, mirbad, v, b);
    st[k] = b ? GRAAL_LINK_NONFINITE : GRAAL_LINK_VALID;
    q[k] = b ? 0 : v;
}

// ---- graal_end_links_best: the same scored links without the materialised output.  A wave per slot of the candidate table (unlisted
// slots return at once) walks the groups of 8 fragments of A from eA that k_ln_mass's waves would cover, through the same ln_group_mass /
// ln_group_quirk, so every fragment pair gets the same Q-rounded term and the int64 sums are the same; the final score stays in the table (tq), then two atomic passes per end.
__device__ __forceinline__ bool lb_listed(const unsigned long long* __restrict__ keys, const int* __restrict__ tf, long long i)
{
    return keys[i] != LN_EMPTY && (tf[i] & 2);
}

__global__ __launch_bounds__(256) void k_lb_mass(long long cap, const unsigned long long* __restrict__ keys, int* __restrict__ tf,
                                                 const int* __restrict__ lab, const LnCtg* __restrict__ ctg, const LnFrag* __restrict__ fr,
                                                 float nfpb, Par par, int quirk, int reach_bp, long long* __restrict__ tq)
{
    const int lane = threadIdx.x & 63;
    const long long W = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (W >= cap || !lb_listed(keys, tf, W)) return;                 // (wave-uniform)
    const unsigned long long key = keys[W];
    const int e_a = (int)(key >> 32), e_b = (int)(key & 0xffffffffull);
    const LnCtg CA = ctg[lab[e_a >> 1]], CB = ctg[lab[e_b >> 1]];
    const LnSide A = ln_side(CA, e_a & 1, true), B = ln_side(CB, e_b & 1, false);
    long long sum = 0, nb = 0;
    for (int g = 0; g * 8 < A.cnt; g++) {
        LnRow r;
        ln_group_row(A, g, fr, reach_bp, r);
        if (__ballot(r.live) == 0ull) break;                         // (the gap grows along the walk of A: no later group is in the window)
        ln_group_mass(r, A, B, fr, nfpb, par, quirk, reach_bp, sum, nb);
    }
    sum = ln_wave_sum(sum);
    nb = ln_wave_sum(nb);
    if (lane == 0) {                                                 // (the slot's only writer in this kernel)
        tq[W] += sum;
        if (nb) tf[W] |= 1;
    }
}

__global__ __launch_bounds__(256) void k_lb_quirk(long long cap, const unsigned long long* __restrict__ keys, int* __restrict__ tf,
                                                  const int* __restrict__ lab, const LnCtg* __restrict__ ctg, const LnFrag* __restrict__ fr,
                                                  float nfpb, Par par, int reach_bp, long long* __restrict__ tq)
{
    const int lane = threadIdx.x & 63;
    const long long W = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (W >= cap || !lb_listed(keys, tf, W)) return;
    const unsigned long long key = keys[W];
    const int e_a = (int)(key >> 32), e_b = (int)(key & 0xffffffffull);
    const LnCtg CA = ctg[lab[e_a >> 1]], CB = ctg[lab[e_b >> 1]];
    if (CA.nmix == 0 && CB.nmix == 0) return;
    const LnSide A = ln_side(CA, e_a & 1, true), B = ln_side(CB, e_b & 1, false);
    long long sum = 0, nb = 0;
    for (int g = 0; g * 8 < A.cnt; g++) ln_group_quirk(A, B, g, fr, nfpb, par, reach_bp, sum, nb);
    sum = ln_wave_sum(sum);
    nb = ln_wave_sum(nb);
    if (lane == 0) {
        tq[W] += sum;
        if (nb) tf[W] |= 1;
    }
}

__global__ void k_lb_init(long long n2, long long* __restrict__ bq, int* __restrict__ be)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n2) { bq[e] = LLONG_MIN; be[e] = INT_MAX; }
}

// k_ln_out per slot: the final Q (mirrors of the reversed contigs added) stays in tq, bit 4 of tf marks a valid link; then the highest Q per end
__global__ void k_lb_out(long long cap, const unsigned long long* __restrict__ keys, int* __restrict__ tf, const int* __restrict__ lab,
                         const long long* __restrict__ mir, const int* __restrict__ mirbad, int quirk, long long* __restrict__ tq,
                         long long* __restrict__ bq)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || !lb_listed(keys, tf, i)) return;
    const int ea = (int)(keys[i] >> 32), eb = (int)(keys[i] & 0xffffffffull);
    long long v = tq[i];
    int b = tf[i] & 1;
    if (quirk) ln_add_mirrors(ea, eb, lab, mir, mirbad, v, b);
    if (b) return;
    tq[i] = v;
    tf[i] |= 4;
    atomicMax(&bq[ea], v);
    atomicMax(&bq[eb], v);
}

// the lowest partner among the valid links that reach an end's highest Q
__global__ void k_lb_arg(long long cap, const unsigned long long* __restrict__ keys, const int* __restrict__ tf, const long long* __restrict__ tq,
                         const long long* __restrict__ bq, int* __restrict__ be)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap || keys[i] == LN_EMPTY || !(tf[i] & 4)) return;
    const int ea = (int)(keys[i] >> 32), eb = (int)(keys[i] & 0xffffffffull);
    if (tq[i] == bq[ea]) atomicMin(&be[ea], eb);
    if (tq[i] == bq[eb]) atomicMin(&be[eb], ea);
}

__global__ void k_lb_norm(long long n2, long long* __restrict__ bq, int* __restrict__ be)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n2 && be[e] == INT_MAX) { be[e] = -1; bq[e] = 0; }
}

// end e heads a mutual link when its best partner p > e has e as ITS best partner, with Q > 0
__global__ void k_lb_flag(long long n2, const long long* __restrict__ bq, const int* __restrict__ be, unsigned char* __restrict__ flag)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n2) return;
    const int p = be[e];
    flag[e] = (p > e && p < n2 && be[p] == (int)e && bq[e] > 0) ? 1 : 0;
}

__global__ void k_lb_gather(long long m, const int* __restrict__ sel, const long long* __restrict__ bq, const int* __restrict__ be,
                            int* __restrict__ ea, int* __restrict__ eb, long long* __restrict__ q)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int e = sel[k];
    ea[k] = e; eb[k] = be[e]; q[k] = bq[e];
}


// The front half of graal_end_links and graal_end_links_best: the records, the count pass, and the table size `cap` for its upper bound
// of the distinct keys.  err: the flags of a corrupt layout (the slots and the sub-fragment records are not to be trusted, nothing
// reads them).
struct LnCount { unsigned err = 0; unsigned long long ctr[3] = {0, 0, 0}, bound = 0, cap = 0; int nb = 1; };

int ln_count(Ctx* h, LayoutRecs& R, int min_frags, int quirk, LnCount& C)
{
    hipStream_t s = h->stream;
    int rc = GRAAL_OK;
    do {
        if ((rc = recs_build(h, R, min_frags)) || (rc = slots_read_err(h, R.L, C.err)) || C.err) break;
        C.nb = stream_blocks(h->nnz);
        if (h->nnz > 0) {
            k_ln_nnz<true><<<C.nb, 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, R.sub, h->stat_frag, R.ctg, h->nfpb, h->par, quirk, 0, nullptr,
                                                nullptr, nullptr, nullptr, nullptr, nullptr, &R.ctr[0], R.L.err);
            STEP_CK(hipGetLastError());
        }
        STEP_CK(hipMemcpyAsync(C.ctr, R.ctr, sizeof C.ctr, hipMemcpyDeviceToHost, s));
        if ((rc = slots_read_err(h, R.L, C.err)) || C.err) break;
        const unsigned long long E = 2ull * C.ctr[2];
        C.bound = std::min<unsigned long long>(C.ctr[0], E * (E > 0 ? E - 1 : 0) / 2);
        C.cap = table_cap(C.bound);
    } while (false);
    return rc;
}

// graal_end_links between score_entry and score_exit: the scored, sorted link table in Lb (m links).  fn names the caller in the
// refusals (why, written into msg); need: the device bytes counted against the budget; mirc_keep, if not null, receives the contact part
// of mirror[C] (n + 3 words) as the insert pass leaves it, before k_ln_mirror adds the mass part into the same array -- int64 sums are
// exact, so the split changes no word of the total (links_boot.h re-forms the contact part per replicate).
int ln_links(Ctx* h, LnBuf* Lb, int min_frags, const char* fn, long long* mirc_keep, LnCount& C, long long& m, const char*& why, char* msg,
             size_t msg_len, unsigned long long& need)
{
    LayoutRecs& R = Lb->R;
    CandTable& T = Lb->T;
    const int n = h->n;
    hipStream_t s = h->stream;
    if (const int rc = recs_reserve(h, R)) return rc;
    const int quirk = (h->mode & GRAAL_MODE_REF_TRANS_ACCU) ? 1 : 0;
    const int mq = quirk && h->n_ubins > 0;
    int rc = GRAAL_OK;
    m = 0;
    do {
        if ((rc = ln_count(h, R, min_frags, quirk, C)) || C.err) break;
        const unsigned long long cap = C.cap, L = C.bound + 1;
        // device memory: the table (key, q, contacts, flags, selection byte per slot), the per-link arrays sized to the bound (keys x2,
        // indices x2, q, contacts, groups x2, bad, ends x2, status) and the hipCUB temp storage of the selection, the sort and the scan
        need = cap * TABLE_SLOT_BYTES + L * (unsigned long long)(8 * 2 + 4 * 2 + 8 + 8 + 8 * 2 + 4 + 4 * 2 + 1);
        size_t b_sel = 0, b_sort = 0, b_scan = 0;
        if (cap < (unsigned long long)INT_MAX) {
            STEP_CK(hipcub::DeviceSelect::Flagged(nullptr, b_sel, hipcub::CountingInputIterator<int>(0), (const unsigned char*)nullptr, (int*)nullptr,
                                                  (unsigned long long*)nullptr, (int)cap, s));
            STEP_CK(hipcub::DeviceRadixSort::SortPairs(nullptr, b_sort, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                       (const int*)nullptr, (int*)nullptr, (int)L, 0, 64, s));
            STEP_CK(hipcub::DeviceScan::ExclusiveSum(nullptr, b_scan, (const long long*)nullptr, (long long*)nullptr, (int)L, s));
        }
        const size_t tneed = std::max(b_sel, std::max(b_sort, b_scan));
        need += tneed;
        if (cap >= (unsigned long long)INT_MAX || need > (unsigned long long)GRAAL_LINKS_MAX_BYTES) {
            snprintf(msg, msg_len, "%s: the candidate table needs %llu bytes (%llu records counted), over the budget of %llu bytes "
                     "(GRAAL_LINKS_MAX_BYTES): use a larger min_frags", fn, need, C.ctr[0], (unsigned long long)GRAAL_LINKS_MAX_BYTES);
            why = msg;
            break;
        }
        STEP_CK(table_reserve(T, cap));
        STEP_CK(table_clear(T, cap, s));
        STEP_CK(group_grow(Lb->lcap, L, Lb->ko, L, Lb->ks, L, Lb->vo, L, Lb->vs, L, Lb->q, L, Lb->c, L, Lb->ch, L, Lb->choff, L, Lb->bad, L, Lb->ea, L,
                           Lb->eb, L, Lb->st, L));
        STEP_CK(scratch_reserve(T, tneed));
        // ---- insert pass, selection of the listed slots, sort by key
        if (h->nnz > 0) {
            k_ln_nnz<false><<<C.nb, 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, R.sub, h->stat_frag, R.ctg, h->nfpb, h->par, quirk, cap, T.keys,
                                                 T.tq, T.tc, T.tf, R.mir, R.mirbad, &R.ctr[0], R.L.err);
            STEP_CK(hipGetLastError());
        }
        if (mirc_keep) STEP_CK(hipMemcpyAsync(mirc_keep, R.mir, sizeof(long long) * (size_t)(n + 3), hipMemcpyDeviceToDevice, s));
        k_ln_flag<<<blocks_for((long long)cap, 256), 256, 0, s>>>(T.keys, T.tf, (long long)cap, T.tsel);
        STEP_CK(hipGetLastError());
        size_t tb = T.stmp.count;
        STEP_CK(hipcub::DeviceSelect::Flagged(T.stmp, tb, hipcub::CountingInputIterator<int>(0), (const unsigned char*)T.tsel, Lb->vo.p, &R.ctr[1],
                                              (int)cap, s));
        STEP_CK(hipMemcpyAsync(C.ctr, R.ctr, sizeof C.ctr, hipMemcpyDeviceToHost, s));
        if ((rc = slots_read_err(h, R.L, C.err)) || C.err) break;
        m = (long long)C.ctr[1];
        if (m == 0) break;
        k_ln_keys<<<blocks_for(m, 256), 256, 0, s>>>(m, T.keys, Lb->vo, Lb->ko);
        STEP_CK(hipGetLastError());
        tb = T.stmp.count;
        STEP_CK(hipcub::DeviceRadixSort::SortPairs(T.stmp.p, tb, Lb->ko.p, Lb->ks.p, Lb->vo.p, Lb->vs.p, (int)m, 0, 64, s));
        k_ln_gather<<<blocks_for(m, 256), 256, 0, s>>>(m, Lb->ks, Lb->vs, T.tq, T.tc, T.tf, R.lab, R.ctg, Lb->q, Lb->c, Lb->bad, Lb->ch, Lb->ea,
                                                       Lb->eb);
        STEP_CK(hipGetLastError());
        tb = T.stmp.count;
        STEP_CK(hipcub::DeviceScan::ExclusiveSum(T.stmp, tb, Lb->ch.p, Lb->choff.p, (int)m, s));
        long long last[2] = {0, 0};
        STEP_CK(hipMemcpyAsync(&last[0], Lb->choff + (m - 1), sizeof(long long), hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(&last[1], Lb->ch + (m - 1), sizeof(long long), hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
        const long long groups = last[0] + last[1];
        if ((groups + 3) / 4 > (long long)INT_MAX) {
            snprintf(msg, msg_len, "%s: %lld wave groups exceed one launch: use a larger min_frags", fn, groups);
            why = msg;
            break;
        }
        // ---- the mass pass, the quirk's passes, the result
        if (groups > 0) {
            k_ln_mass<<<(unsigned)((groups + 3) / 4), 256, 0, s>>>(m, groups, Lb->choff, Lb->ch, Lb->ea, Lb->eb, R.lab, R.ctg, R.fr, h->nfpb, h->par,
                                                                 quirk, reach_bp(h), Lb->q, Lb->bad);
            STEP_CK(hipGetLastError());
        }
        if (mq) {
            k_ln_mirror<<<h->n_ubins, 256, 0, s>>>(n, h->d_ubins, R.L.slot, R.lab, R.ctg, R.fr, h->nfpb, h->par, R.mir, R.mirbad);
            STEP_CK(hipGetLastError());
            if (groups > 0)
                k_ln_quirk<<<(unsigned)((groups + 3) / 4), 256, 0, s>>>(m, groups, Lb->choff, Lb->ch, Lb->ea, Lb->eb, R.lab, R.ctg, R.fr, h->nfpb,
                                                                      h->par, reach_bp(h), Lb->q, Lb->bad);
            STEP_CK(hipGetLastError());
        }
        k_ln_out<<<blocks_for(m, 256), 256, 0, s>>>(m, Lb->ea, Lb->eb, R.lab, R.mir, R.mirbad, mq, Lb->q, Lb->bad, Lb->st);
        STEP_CK(hipGetLastError());
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    return rc;
}

} // namespace

extern "C" {

int graal_end_links(graal_ctx* h, int32_t min_frags, int64_t* n_links)
{
    if (!h || !n_links) return GRAAL_E_ARG;
    if (min_frags < 1) return fail(h, GRAAL_E_ARG, "graal_end_links: min_frags must be >= 1");
    if (const int rc = score_entry(h, "graal_end_links")) return rc;
    *n_links = 0;
    if (!h->ln) h->ln = new LnBuf();
    LnBuf* Lb = h->ln;
    Lb->n_links = -1;
    Lb->boot_links = -1;                                             // (a bootstrap's columns describe the table this call replaces)
    if (h->n < 1) { Lb->n_links = 0; return GRAAL_OK; }
    LnCount C;
    long long m = 0;
    const char* why = nullptr;
    char msg[320];
    unsigned long long need = 0;
    const int rc = ln_links(h, Lb, min_frags, "graal_end_links", nullptr, C, m, why, msg, sizeof msg, need);
    if (const int r = score_exit(h, "graal_end_links", rc, why, C.err)) return r;
    Lb->n_links = m;
    *n_links = m;
    return GRAAL_OK;
}

int graal_end_links_fetch(graal_ctx* h, int32_t* end_a, int32_t* end_b, int64_t* q, int64_t* contacts, uint8_t* status, int64_t cap)
{
    if (!h || !end_a || !end_b || !q || !contacts || !status) return GRAAL_E_ARG;
    LnBuf* Lb = h->ln;
    if (!Lb || Lb->n_links < 0) return fail(h, GRAAL_E_STATE, "graal_end_links_fetch: call graal_end_links first");
    const long long m = Lb->n_links;
    if (cap < m) return fail(h, GRAAL_E_ARG, "graal_end_links_fetch: cap is smaller than the number of links");
    if (m == 0) return GRAAL_OK;
    CK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    CK(hipMemcpyAsync(end_a, Lb->ea, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(end_b, Lb->eb, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(q, Lb->q, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(contacts, Lb->c, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(status, Lb->st, (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    return GRAAL_OK;
}

int graal_end_links_best(graal_ctx* h, int32_t min_frags, int32_t* best_end, int64_t* best_q, int64_t* n_mutual)
{
    if (!h || !best_end || !best_q || !n_mutual) return GRAAL_E_ARG;
    if (min_frags < 1) return fail(h, GRAAL_E_ARG, "graal_end_links_best: min_frags must be >= 1");
    if (const int rc = score_entry(h, "graal_end_links_best")) return rc;
    *n_mutual = 0;
    const int n = h->n;
    const long long n2 = 2ll * n;
    if (!h->ln) h->ln = new LnBuf();
    LnBuf* Lb = h->ln;
    LayoutRecs& R = Lb->R;
    CandTable& T = Lb->T;
    Lb->n_mutual = -1;
    if (n < 1) { Lb->n_mutual = 0; return GRAAL_OK; }
    hipStream_t s = h->stream;
    if (const int rc = recs_reserve(h, R)) return rc;
    const int quirk = (h->mode & GRAAL_MODE_REF_TRANS_ACCU) ? 1 : 0;
    const int mq = quirk && h->n_ubins > 0;
    int rc = GRAAL_OK;
    LnCount C;
    long long m = 0;
    const char* why = nullptr;
    char msg[320];
    do {
        if ((rc = ln_count(h, R, min_frags, quirk, C)) || C.err) break;
        const unsigned long long cap = C.cap;
        // device memory: the table (key, q, contacts, flags, selection byte per slot), the per-end arrays (best q, best partner, flag,
        // selected end, mutual end_a / end_b / q) and the hipCUB temp storage of the selection over the ends -- no per-link arrays
        unsigned long long need = cap * TABLE_SLOT_BYTES + (unsigned long long)n2 * (8 + 4 + 1 + 4 + 4 + 4 + 8);
        size_t b_sel = 0;
        STEP_CK(hipcub::DeviceSelect::Flagged(nullptr, b_sel, hipcub::CountingInputIterator<int>(0), (const unsigned char*)nullptr, (int*)nullptr,
                                              (unsigned long long*)nullptr, (int)n2, s));
        need += b_sel;
        if (cap >= (unsigned long long)INT_MAX || (cap + 3) / 4 >= (unsigned long long)INT_MAX || need > (unsigned long long)GRAAL_LINKS_MAX_BYTES) {
            snprintf(msg, sizeof msg, "graal_end_links_best: the candidate table needs %llu bytes (%llu records counted), over the budget of %llu "
                     "bytes (GRAAL_LINKS_MAX_BYTES): use a larger min_frags", need, C.ctr[0], (unsigned long long)GRAAL_LINKS_MAX_BYTES);
            why = msg;
            break;
        }
        STEP_CK(table_reserve(T, cap));
        STEP_CK(group_grow(Lb->bcap, n2, Lb->bq, n2, Lb->be, n2, Lb->bflag, n2, Lb->bsel, n2, Lb->mea, n2, Lb->meb, n2, Lb->mq, n2));
        STEP_CK(scratch_reserve(T, b_sel));
        STEP_CK(table_clear(T, cap, s));
        // ---- insert pass, then the scores in place: mass, the quirk's passes, mirrors and status
        if (h->nnz > 0) {
            k_ln_nnz<false><<<C.nb, 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, R.sub, h->stat_frag, R.ctg, h->nfpb, h->par, quirk, cap, T.keys,
                                                 T.tq, T.tc, T.tf, R.mir, R.mirbad, &R.ctr[0], R.L.err);
            STEP_CK(hipGetLastError());
        }
        const unsigned wblocks = (unsigned)((cap + 3) / 4);          // a wave per slot, 4 waves per block
        k_lb_mass<<<wblocks, 256, 0, s>>>((long long)cap, T.keys, T.tf, R.lab, R.ctg, R.fr, h->nfpb, h->par, quirk, reach_bp(h), T.tq);
        STEP_CK(hipGetLastError());
        if (mq) {
            k_ln_mirror<<<h->n_ubins, 256, 0, s>>>(n, h->d_ubins, R.L.slot, R.lab, R.ctg, R.fr, h->nfpb, h->par, R.mir, R.mirbad);
            STEP_CK(hipGetLastError());
            k_lb_quirk<<<wblocks, 256, 0, s>>>((long long)cap, T.keys, T.tf, R.lab, R.ctg, R.fr, h->nfpb, h->par, reach_bp(h), T.tq);
            STEP_CK(hipGetLastError());
        }
        // ---- per end: the highest Q, then the lowest partner that reaches it, then the mutual links
        k_lb_init<<<blocks_for(n2, 256), 256, 0, s>>>(n2, Lb->bq, Lb->be);
        k_lb_out<<<blocks_for((long long)cap, 256), 256, 0, s>>>((long long)cap, T.keys, T.tf, R.lab, R.mir, R.mirbad, mq, T.tq, Lb->bq);
        k_lb_arg<<<blocks_for((long long)cap, 256), 256, 0, s>>>((long long)cap, T.keys, T.tf, T.tq, Lb->bq, Lb->be);
        k_lb_norm<<<blocks_for(n2, 256), 256, 0, s>>>(n2, Lb->bq, Lb->be);
        k_lb_flag<<<blocks_for(n2, 256), 256, 0, s>>>(n2, Lb->bq, Lb->be, Lb->bflag);
        STEP_CK(hipGetLastError());
        size_t tb = T.stmp.count;
        STEP_CK(hipcub::DeviceSelect::Flagged(T.stmp, tb, hipcub::CountingInputIterator<int>(0), (const unsigned char*)Lb->bflag, Lb->bsel.p,
                                              &R.ctr[1], (int)n2, s));
        STEP_CK(hipMemcpyAsync(C.ctr, R.ctr, sizeof C.ctr, hipMemcpyDeviceToHost, s));
        if ((rc = slots_read_err(h, R.L, C.err)) || C.err) break;
        m = (long long)C.ctr[1];
        if (m > 0) {
            k_lb_gather<<<blocks_for(m, 256), 256, 0, s>>>(m, Lb->bsel, Lb->bq, Lb->be, Lb->mea, Lb->meb, Lb->mq);
            STEP_CK(hipGetLastError());
        }
        STEP_CK(hipMemcpyAsync(best_end, Lb->be, sizeof(int) * (size_t)n2, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(best_q, Lb->bq, sizeof(long long) * (size_t)n2, hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    if (const int r = score_exit(h, "graal_end_links_best", rc, why, C.err)) return r;
    Lb->n_mutual = m;
    *n_mutual = m;
    return GRAAL_OK;
}

int graal_end_links_mutual_fetch(graal_ctx* h, int32_t* end_a, int32_t* end_b, int64_t* q, int64_t cap)
{
    if (!h || !end_a || !end_b || !q) return GRAAL_E_ARG;
    LnBuf* Lb = h->ln;
    if (!Lb || Lb->n_mutual < 0) return fail(h, GRAAL_E_STATE, "graal_end_links_mutual_fetch: call graal_end_links_best first");
    const long long m = Lb->n_mutual;
    if (cap < m) return fail(h, GRAAL_E_ARG, "graal_end_links_mutual_fetch: cap is smaller than the number of mutual links");
    if (m == 0) return GRAAL_OK;
    CK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    CK(hipMemcpyAsync(end_a, Lb->mea, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(end_b, Lb->meb, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(q, Lb->mq, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    return GRAAL_OK;
}

} // extern "C"
