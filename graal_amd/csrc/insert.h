// insert.h -- the likelihood every insertion of a small contig into a junction would add, for every (piece, junction, orientation) the
// contacts support (graal_insertions).  Included by graal_hip.hip after links.h (it uses LayoutRecs with recs_reserve / recs_build, the
// records LnSub / LnFrag / LnCtg, ln_slot, ln_pair_mass, ln_quirk_pair, ln_mirror_q, k_ln_mirror, k_ln_flag and k_ln_keys, wave_runs.h's run_sums, and
// score_common.h's score_entry, score_exit, STEP_CK, stream_blocks and CandTable).
//
// A PIECE is a linear contig P of 1 .. max_piece_frags fragments; a TARGET junction is a fragment f with next[f] = g != -1 of a linear
// contig T != P.  The inserted layout cuts T between f and g into T1 (.. f) and T2 (g ..) and writes T1, P, T2 as one contig: T1 and T2
// keep T's direction, P enters as it is (rev 0: its head next to f) or reversed (rev 1: its tail next to f); integer bp offsets as m_paste
// writes them (P's fragments start at end(f) + their offset in P, T2's are shifted by len(P) = P's l_cont_bp), then the float32 centres.
// I(P, f, rev) = logL(inserted) - logL(current) in the exact arithmetic with the roundings of junctions.h / links.h:
//   - P x T pairs: from their trans price to their cis price in the inserted layout;
//   - T1 x T2 pairs: from their cis price at distance d to their cis price at d + len(P) (rippe: v_inter past d_max);
//   - pairs inside P, T1, T2: unchanged; a contact's term rounded to Q once, a fragment pair's mass once; int64 sums;
//   - GRAAL_MODE_REF_TRANS_ACCU with mixed bins: the P x T pairs beyond the window with a mixed bin, and for rev 1 P's mirror (links.h)
//     less its part on T.
// Decomposition of the contact terms.  For a P x T contact at a junction where its inserted distance is >= d_max the term is the FAR term
// ob * (ln ex_plain - ln ex_trans) (zero unless the trans indexing differs): so every candidate (P, f, rev) gets the far terms of ALL P x T
// contacts, a per-(P, T) sum, plus, for each contact inside the window at its junction, Q(term) - Q(far term) -- the same Q-rounded terms.
// Kernels, all on the engine's stream:
//   recs_build (k_jn_count / scan / k_ln_prep, min_frags 1) / k_in_piece -- links.h's slots and records; a contig record's `elig` then marks a piece;
//   row offsets of the contact list by row, for k_in_shift: the engine's own row index when the list was uploaded sorted by row (built
//                 once per upload, k_rowptr); the upload takes the list in any order: k_in_unsorted checks it, an unsorted list is
//                 radix-sorted by row into a permutation first and k_rowptr runs over that copy;
//   k_in_nnz<COUNT> -- streams the contact list, 64 contacts per wave.  For a contact between x of a piece and y of a target the junctions
//                 that keep it inside the window are a run of slots on each side of y: the wave walks them outward (both pieces of a
//                 pair, both orientations, both sides) until every lane's inserted gap passed reach_bp, emitting (f << 32 | head << 1 | rev)
//                 when the inserted distance is < d_max.  Run sums as k_ln_nnz, count pass then 64-bit CAS insert pass.  Under the indexing
//                 mode with mixed bins it also sums the far terms and the mirror's contact part on T per (P label, T label) (a second
//                 table) and the contact part of mirror[P] per piece;
//   k_ln_flag, DeviceSelect::Flagged, k_ln_keys, radix sort, k_in_gather -- the listed keys in (f, P head, rev) order;
//   k_in_lead  -- per candidate the first candidate at the same junction with the same len(P): the T1 x T2 term is computed once for them;
//   k_in_mass  -- a wave per candidate: lanes 8 x 8 fragment pairs (P's fragments x T's walked outward from the junction on each side),
//                 stopping when every pair has left the window;
//   k_in_shift -- a wave per leading candidate: the T1 x T2 pairs straddling f within the window (mass as k_in_mass's tiles; contacts from
//                 the rows of the window's fragments);
//   k_ln_mirror, k_in_quirk -- only under the indexing mode with mixed bins: mirror[P] (one block per mixed bin of a piece), and a wave per
//                 candidate over P x all of T (ln_quirk_pair);
//   k_in_out   -- the sum and a status byte.
#pragma once

namespace {

struct InBuf {
    LayoutRecs R;                                                    // (its own instance: nothing shared with graal_end_links' calls)
    CandTable T;
    DevBuf<long long> rowptr; size_t rcap = 0;                       // row offsets (S + 1) when the engine has none for this list
    DevBuf<unsigned> uns;                                            // the contact list is not sorted by row
    DevBuf<int> srow, pin, perm; DevBuf<void> ptmp; size_t pcap = 0; // its sort by row
    // the candidate table (T), the (P, T) table and the per-candidate arrays grow to the largest size a call needed (within GRAAL_LINKS_MAX_BYTES)
    DevBuf<unsigned long long> keys2; DevBuf<long long> pf, pm; DevBuf<int> pb; size_t cap2 = 0;
    DevBuf<unsigned long long> ko, ks; DevBuf<int> vo, vs;
    DevBuf<long long> q, c, sh; DevBuf<int> bad, shbad, lead, piece, after;
    DevBuf<unsigned char> rev, st;
    size_t lcap = 0;
    long long n_out = -1;                                            // -1: no result to fetch
};

void in_free(InBuf* b) { delete b; }

// after k_ln_prep (min_frags 1: a record's elig = linear): a contig record's elig marks a PIECE (linear, 1 .. max_piece_frags fragments)
__global__ void k_in_piece(int nl, int max_piece, LnCtg* __restrict__ ctg)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < nl) ctg[c].elig = (ctg[c].elig && ctg[c].cnt >= 1 && ctg[c].cnt <= max_piece) ? 1 : 0;
}

// flag 1 when some contact's row is larger than the next one's
__global__ void k_in_unsorted(const int* __restrict__ row, long long nnz, unsigned* __restrict__ flag)
{
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k + 1 < nnz; k += (long long)gridDim.x * blockDim.x)
        if (row[k] > row[k + 1]) { atomicOr(flag, 1u); return; }
}

__global__ void k_in_iota(int m, int* __restrict__ v)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < m) v[k] = k;
}

__device__ __forceinline__ unsigned long long in_key(int f, int head, int rev)
{
    return ((unsigned long long)(unsigned)f << 32) | (((unsigned)head << 1) | (unsigned)rev);
}

// The contact pass.  COUNT: count the records a wave would insert into each table (after its run sums).  Otherwise insert them, and sum
// the contact part of mirror[P] per piece (mq only).
template <bool COUNT>
__global__ __launch_bounds__(256) void k_in_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt, long long nnz,
                                                const LnSub* __restrict__ sub, const Stat* __restrict__ stat, const LnCtg* __restrict__ ctg,
                                                const LnFrag* __restrict__ fr, const int* __restrict__ slot_of, float nfpb, Par par, int quirk,
                                                int mq, int reach, unsigned long long cap, unsigned long long* __restrict__ keys,
                                                long long* __restrict__ tq, long long* __restrict__ tc, int* __restrict__ tf,
                                                unsigned long long cap2, unsigned long long* __restrict__ keys2, long long* __restrict__ pf,
                                                long long* __restrict__ pm, int* __restrict__ pb, long long* __restrict__ mir,
                                                int* __restrict__ mirbad, unsigned long long* __restrict__ ctr, unsigned* __restrict__ err)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    unsigned long long n_wave = 0, n_wave2 = 0;
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {   // (wave-uniform bounds: the run sums need the whole wave)
        const long long k = k0 + lane;
        LnSub X = {-1, -1, 0, 0, 0, 0, 0, 0}, Y = X;
        LnCtg CX = {}, CY = {};
        bool diff = false;
        if (k < nnz) {
            X = sub[row[k]]; Y = sub[col[k]];
            diff = X.label != Y.label && X.label >= 0 && Y.label >= 0;
            if (diff) { CX = ctg[X.label]; CY = ctg[Y.label]; }
        }
        // direction 0: X in the piece, Y in the target; direction 1 the other way round
        const bool d0 = diff && CX.elig && ln_elig(Y.meta) && CY.cnt >= 2;
        const bool d1 = diff && CY.elig && ln_elig(X.meta) && CX.cnt >= 2;
        const bool x_low = X.frag < Y.frag;
        const LnSub& lo = x_low ? X : Y;
        const bool lo_piece = diff && (x_low ? CX.elig : CY.elig) && ln_mixed(lo.meta);
        if (__ballot(d0 || d1 || (mq && lo_piece)) == 0ull) continue;
        const double ob = k < nnz ? (double)__int_as_float(cnt[k]) : 0.0;
        const int own_x = X.acc & 0xffff, own_y = Y.acc & 0xffff;
        const int prod = own_x * own_y;
        int prod_t = prod, prod_f = prod;                            // the current trans indexing, and with the lower bin flipped
        if (quirk && diff) {
            const int own_l = lo.acc & 0xffff, last_l = lo.acc >> 16, other = x_low ? own_y : own_x;
            prod_t = (ln_fwd(lo.meta) ? own_l : last_l) * other;
            prod_f = (ln_fwd(lo.meta) ? last_l : own_l) * other;
        }
        const float et = par.v_inter * ((float)prod_t / nfpb);
        const double ln_et = mm_ln(et);
        long long m_term = 0, far = 0;
        bool m_bad = false, far_bad = false;
        if (mq && lo_piece && prod_f != prod_t) {
            const float ef = par.v_inter * ((float)prod_f / nfpb);
            m_term = to_q(ob * (mm_ln(ef) - ln_et));
            if (m_term == Q_BAD) { m_bad = true; m_term = 0; }
        }
        if (mq && (d0 || d1) && prod_t != prod) {
            far = to_q(ob * (mm_ln(par.v_inter * ((float)prod / nfpb)) - ln_et));
            if (far == Q_BAD) { far_bad = true; far = 0; }
        }
        if (mq) {
            if (!COUNT) {                                            // mirror[P]'s contacts, summed per run of the lower bin's piece
                const unsigned long long mk = (lo_piece && (m_term != 0 || m_bad)) ? (unsigned long long)lo.label : LN_EMPTY;
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
            // per (P label, T label): the far terms of every P x T contact and the mirror's contact part on T
#pragma unroll 1
            for (int d = 0; d < 2; d++) {
                const bool ok = d ? d1 : d0;
                const bool p_low = d ? !x_low : x_low;               // the lower bin is the piece's
                long long v0 = ok ? far : 0, v1 = (ok && p_low) ? m_term : 0;
                long long v2 = ok ? (far_bad ? 1 : 0) + ((p_low && m_bad) ? (1ll << 32) : 0) : 0;   // (counts: far | mirror << 32)
                const unsigned long long key = (ok && (v0 != 0 || v1 != 0 || v2 != 0))
                    ? ((unsigned long long)(unsigned)(d ? Y.label : X.label) << 32) | (unsigned)(d ? X.label : Y.label) : LN_EMPTY;
                if (__ballot(key != LN_EMPTY) == 0ull) continue;
                bool tail;
                run_sums(key, tail, v0, v1, v2);
                const bool rec = tail && key != LN_EMPTY;
                if (COUNT) {
                    n_wave2 += (unsigned long long)__popcll(__ballot(rec));
                } else if (rec) {
                    const long long i = ln_slot(keys2, cap2, key, err);
                    if (i >= 0) {
                        if (v0 != 0) atomicAdd((unsigned long long*)&pf[i], (unsigned long long)v0);
                        if (v1 != 0) atomicAdd((unsigned long long*)&pm[i], (unsigned long long)v1);
                        if (v2 != 0) atomicOr(&pb[i], ((v2 & 0xffffffffll) ? 1 : 0) | ((v2 >> 32) ? 2 : 0));
                    }
                }
            }
        }
        if (__ballot(d0 || d1) == 0ull) continue;
        Stat SX = {}, SY = {};
        if (d0 || d1) { SX = stat[X.frag]; SY = stat[Y.frag]; }
#pragma unroll 1
        for (int cmb = 0; cmb < 8; cmb++) {
            const int d = cmb >> 2, rv = (cmb >> 1) & 1, side = cmb & 1;   // side 0: y in T1 (junctions from y on); side 1: y in T2
            const bool ok = d ? d1 : d0;
            if (__ballot(ok) == 0ull) continue;
            const LnSub& xs = d ? Y : X;
            const LnSub& ys = d ? X : Y;
            const Stat& Sx = d ? SY : SX;
            const Stat& Sy = d ? SX : SY;
            const LnCtg& CP = d ? CY : CX;
            const LnCtg& CT = d ? CX : CY;
            int off = 0, pg = 0, pos_y = 0;
            float cy = 0.0f;
            if (ok) {
                off = rv ? CP.lbp - xs.start - xs.len : xs.start;    // x's offset from P's end next to f
                pg = CP.lbp - off - xs.len;                          // x's gap to P's end next to g
                pos_y = slot_of[ys.frag] - CT.first;
                cy = centre_kb(side ? ys.start + CP.lbp : ys.start, ln_fwd(ys.meta), Sy, ln_k(ys.meta));
            }
            const bool fx = ln_fwd(xs.meta) != (rv != 0);
            for (int t = 0; ; t++) {
                const int j = side ? pos_y - 1 - t : pos_y + t;     // f's position in T
                bool live = ok && j >= 0 && j <= CT.cnt - 2;
                int O = 0, ff = 0;
                if (live) {
                    const LnFrag F = fr[CT.first + j];
                    O = F.start + F.len; ff = F.frag;
                    const long long gap = side ? (long long)ys.start - O + pg : (long long)O + off - (ys.start + ys.len);
                    live = gap <= reach;
                }
                if (__ballot(live) == 0ull) break;                   // (the inserted gap grows along the walk)
                unsigned long long key = LN_EMPTY;
                long long q = 0, n_in = 0, fl = 0;
                if (live) {
                    const float cx = centre_kb(O + off, fx, Sx, ln_k(xs.meta));
                    const float sd = fabsf(cy - cx);
                    if (sd < par.d_max) {                            // (beyond it the term is the far term: in the (P, T) sum)
                        const float exn = rippe(sd, par) * ((float)prod / nfpb);
                        const long long tr = to_q(ob * (mm_ln(exn) - ln_et));
                        const bool bad = tr == Q_BAD;
                        q = bad ? 0 : tr - far;
                        key = in_key(ff, CP.head, rv);
                        n_in = (long long)llrint(ob);
                        fl = (bad ? 1 : 0) + (1ll << 32);
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
                        atomicOr(&tf[i], ((fl & 0xffffffffll) ? 1 : 0) | 2);
                    }
                }
            }
        }
    }
    if (COUNT && lane == 0) {
        if (n_wave) atomicAdd(&ctr[0], n_wave);
        if (n_wave2) atomicAdd(&ctr[3], n_wave2);
    }
}

__global__ void k_in_gather(long long m, const unsigned long long* __restrict__ ks, const int* __restrict__ vs, const long long* __restrict__ tq,
                            const long long* __restrict__ tc, const int* __restrict__ tf, long long* __restrict__ q, long long* __restrict__ c,
                            int* __restrict__ bad, long long* __restrict__ sh, int* __restrict__ shbad, int* __restrict__ piece,
                            int* __restrict__ after, unsigned char* __restrict__ rev)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = vs[k];
    const unsigned long long key = ks[k];
    after[k] = (int)(key >> 32); piece[k] = (int)((key & 0xffffffffull) >> 1); rev[k] = (unsigned char)(key & 1);
    q[k] = tq[i]; c[k] = tc[i]; bad[k] = tf[i] & 1;
    sh[k] = 0; shbad[k] = 0;
}

// the first candidate at the same junction whose piece has the same bp length (the candidates of a junction are consecutive)
__global__ void k_in_lead(long long m, const int* __restrict__ piece, const int* __restrict__ after, const int* __restrict__ lab,
                          const LnCtg* __restrict__ ctg, int* __restrict__ lead)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int f = after[k], lbp = ctg[lab[piece[k]]].lbp;
    long long s = k;
    while (s > 0 && after[s - 1] == f) s--;
    long long j = s;
    while (j < k && ctg[lab[piece[j]]].lbp != lbp) j++;
    lead[k] = (int)j;
}

// a candidate's geometry: the junction (slot of f, end of f in bp), T's slots, P's record
struct InCand { int sf, O, first, last, rv; LnCtg P; };

__device__ __forceinline__ InCand in_cand(int f, int head, int rv, const int* __restrict__ slot_of, const int* __restrict__ lab,
                                          const LnCtg* __restrict__ ctg, const LnFrag* __restrict__ fr)
{
    InCand c;
    const LnCtg T = ctg[lab[f]];
    c.sf = slot_of[f];
    const LnFrag F = fr[c.sf];
    c.O = F.start + F.len;
    c.first = T.first; c.last = T.first + T.cnt - 1;
    c.rv = rv;
    c.P = ctg[lab[head]];
    return c;
}

// P x T mass: a wave per candidate; lanes 8 x 8 (fragment of P, fragment of T) pairs, T walked from f back (T1) and from g on (T2)
__global__ __launch_bounds__(256) void k_in_mass(long long m, const int* __restrict__ piece, const int* __restrict__ after,
                                                 const unsigned char* __restrict__ revs, const int* __restrict__ slot_of,
                                                 const int* __restrict__ lab, const LnCtg* __restrict__ ctg, const LnFrag* __restrict__ fr,
                                                 float nfpb, Par par, int quirk, int reach, long long* __restrict__ q, int* __restrict__ bad)
{
    const int lane = threadIdx.x & 63;
    const long long W = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (W >= m) return;
    const InCand C = in_cand(after[W], piece[W], revs[W], slot_of, lab, ctg, fr);
    const int jl = lane & 7;
    long long sum = 0, nb = 0;
    for (int g = 0; g * 8 < C.P.cnt; g++) {
        const int i = g * 8 + (lane >> 3);
        const bool live = i < C.P.cnt;
        LnFrag x;
        int off = 0, pg = 0;
        bool fx = false;
        if (live) {
            x = fr[C.P.first + i];
            off = C.rv ? C.P.lbp - x.start - x.len : x.start;
            pg = C.P.lbp - off - x.len;
            fx = (x.fwd != 0) != (C.rv != 0);
        }
        for (int side = 0; side < 2; side++) {
            for (int j0 = 0; ; j0 += 8) {
                const int ys = side ? C.sf + 1 + j0 + jl : C.sf - j0 - jl;
                bool in = live && (side ? ys <= C.last : ys >= C.first);
                LnFrag y;
                if (in) {
                    y = fr[ys];
                    const long long gap = side ? (long long)y.start - C.O + pg : (long long)C.O + off - (y.start + y.len);
                    in = gap <= reach;
                }
                if (__ballot(in) == 0ull) break;                     // (the inserted gap grows along the walk)
                if (in) {
                    const long long t = to_q_fast(ln_pair_mass(x, C.O + off, fx, y, side ? y.start + C.P.lbp : y.start, y.fwd != 0, nfpb, par,
                                                               quirk));
                    if (t == Q_BAD) nb++; else sum -= t;
                }
            }
        }
    }
    sum = ln_wave_sum(sum);
    nb = ln_wave_sum(nb);
    if (lane == 0) {                                                 // (the candidate's only writer in this kernel)
        q[W] += sum;
        bad[W] += (int)nb;
    }
}

// mass term of T1 x T2 fragment pair (x before the junction, y after it) when y moves by lbp bp: sum of ex(d + lbp) - ex(d), cis both
__device__ __forceinline__ double in_shift_mass(const LnFrag& x, const LnFrag& y, int lbp, float nfpb, const Par& par)
{
    double acc = 0.0;
    for (int a = 0; a < x.st.n; a++) {
        const float ca = centre_kb(x.start, x.fwd != 0, x.st, a);
        const int ax = stat_accu(x.st, a);
        for (int b = 0; b < y.st.n; b++) {
            const float norm = (float)(ax * stat_accu(y.st, b)) / nfpb;
            const float e1 = rippe(fabsf(centre_kb(y.start + lbp, y.fwd != 0, y.st, b) - ca), par) * norm;
            const float e0 = rippe(fabsf(centre_kb(y.start, y.fwd != 0, y.st, b) - ca), par) * norm;
            acc += (double)e1 - (double)e0;
        }
    }
    return acc;
}

// T1 x T2: a wave per leading candidate (lead[k] == k).  Mass: groups of 8 fragments walked back from f x tiles of 8 walked on from g, while
// the current gap is within reach.  Contacts: the rows of the fragments within reach on either side, the partner on the other side.
__global__ __launch_bounds__(256) void k_in_shift(long long m, const int* __restrict__ lead, const int* __restrict__ piece, const int* __restrict__ after,
                                                  const int* __restrict__ slot_of, const int* __restrict__ lab, const LnCtg* __restrict__ ctg,
                                                  const LnFrag* __restrict__ fr, const LnSub* __restrict__ sub, const Stat* __restrict__ stat,
                                                  const int* __restrict__ sub_ids, const long long* __restrict__ rowptr, const int* __restrict__ perm,
                                                  const int* __restrict__ col, const int* __restrict__ cnt, float nfpb, Par par, int reach,
                                                  long long* __restrict__ sh, int* __restrict__ shbad)
{
    const int lane = threadIdx.x & 63;
    const long long W = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (W >= m || lead[W] != (int)W) return;                         // (wave-uniform)
    const int f = after[W];
    const InCand C = in_cand(f, piece[W], 0, slot_of, lab, ctg, fr);
    const int lbp = C.P.lbp, labT = lab[f];
    const int jl = lane & 7;
    long long sum = 0, nb = 0;
    for (int g = 0; ; g++) {
        const int xs = C.sf - g * 8 - (lane >> 3);
        bool live = xs >= C.first;
        LnFrag x;
        long long gx = 0;
        if (live) { x = fr[xs]; gx = (long long)C.O - (x.start + x.len); live = gx <= reach; }
        if (__ballot(live) == 0ull) break;
        for (int j0 = 0; ; j0 += 8) {
            const int ys = C.sf + 1 + j0 + jl;
            bool in = live && ys <= C.last;
            LnFrag y;
            if (in) { y = fr[ys]; in = gx + ((long long)y.start - C.O) <= reach; }
            if (__ballot(in) == 0ull) break;
            if (in) {
                const long long t = to_q_fast(in_shift_mass(x, y, lbp, nfpb, par));
                if (t == Q_BAD) nb++; else sum -= t;
            }
        }
    }
    for (int side = 0; side < 2; side++) {
        for (int s = side ? C.sf + 1 : C.sf; side ? s <= C.last : s >= C.first; s += side ? 1 : -1) {
            const LnFrag z = fr[s];
            if ((side ? (long long)z.start - C.O : (long long)C.O - (z.start + z.len)) > reach) break;
            int4 ids = make_int4(z.frag, 0, 0, 1);
            if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[z.frag];
            for (int kz = 0; kz < z.st.n; kz++) {
                const int sz = sel3(ids.x, ids.y, ids.z, kz);
                const float cz0 = centre_kb(z.start, z.fwd != 0, z.st, kz);
                const float cz1 = side ? centre_kb(z.start + lbp, z.fwd != 0, z.st, kz) : cz0;
                const int az = stat_accu(z.st, kz);
                for (long long r0 = rowptr[sz] + lane; r0 < rowptr[sz + 1]; r0 += 64) {
                    const long long r = perm ? (long long)perm[r0] : r0;   // (the list's own order, or its sort by row)
                    const LnSub Y = sub[col[r]];
                    if (Y.label != labT || Y.frag < 0) continue;
                    const int sy = slot_of[Y.frag];
                    if (side ? sy > C.sf : sy <= C.sf) continue;     // (the partner on the other side of the junction)
                    const Stat SY = stat[Y.frag];
                    const float cy0 = centre_kb(Y.start, ln_fwd(Y.meta), SY, ln_k(Y.meta));
                    const float sd0 = fabsf(cy0 - cz0);
                    if (sd0 >= par.d_max && par.v_inter >= 0.0f) continue;   // (v_inter before and after: the distance only grows)
                    const float cy1 = side ? cy0 : centre_kb(Y.start + lbp, ln_fwd(Y.meta), SY, ln_k(Y.meta));
                    const float norm = (float)(az * (Y.acc & 0xffff)) / nfpb;
                    const float e0 = rippe(sd0, par) * norm, e1 = rippe(fabsf(cy1 - cz1), par) * norm;
                    const long long t = to_q((double)__int_as_float(cnt[r]) * (mm_ln(e1) - mm_ln(e0)));
                    if (t == Q_BAD) nb++; else sum += t;
                }
            }
        }
    }
    sum = ln_wave_sum(sum);
    nb = ln_wave_sum(nb);
    if (lane == 0) { sh[W] = sum; shbad[W] = (int)nb; }
}

// GRAAL_MODE_REF_TRANS_ACCU with mixed bins: a wave per candidate over P x ALL of T -- the pairs beyond the window with a mixed bin, and
// for rev 1 the mirror's mass part on T (ln_quirk_pair, as k_ln_quirk).  Candidates whose two contigs hold no mixed bin return at once.
__global__ __launch_bounds__(256) void k_in_quirk(long long m, const int* __restrict__ piece, const int* __restrict__ after,
                                                  const unsigned char* __restrict__ revs, const int* __restrict__ slot_of,
                                                  const int* __restrict__ lab, const LnCtg* __restrict__ ctg, const LnFrag* __restrict__ fr,
                                                  float nfpb, Par par, int reach, long long* __restrict__ q, int* __restrict__ bad)
{
    const int lane = threadIdx.x & 63;
    const long long W = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (W >= m) return;
    const int f = after[W];
    const InCand C = in_cand(f, piece[W], revs[W], slot_of, lab, ctg, fr);
    if (C.P.nmix == 0 && ctg[lab[f]].nmix == 0) return;
    const int jl = lane & 7;
    long long sum = 0, nb = 0;
    for (int g = 0; g * 8 < C.P.cnt; g++) {
        const int i = g * 8 + (lane >> 3);
        if (i >= C.P.cnt) continue;
        const LnFrag x = fr[C.P.first + i];
        const int off = C.rv ? C.P.lbp - x.start - x.len : x.start, pg = C.P.lbp - off - x.len;
        const bool mx = !stat_uniform(x.st);
        for (int ys = C.first + jl; ys <= C.last; ys += 8) {
            const LnFrag y = fr[ys];
            if (!mx && stat_uniform(y.st)) continue;
            const long long gap = ys <= C.sf ? (long long)C.O + off - (y.start + y.len) : (long long)y.start - C.O + pg;
            ln_quirk_pair(x, y, gap > reach, C.rv != 0, false, nfpb, par, sum, nb);
        }
    }
    sum = ln_wave_sum(sum);
    nb = ln_wave_sum(nb);
    if (lane == 0) {
        if (sum != 0) atomicAdd((unsigned long long*)&q[W], (unsigned long long)sum);
        if (nb != 0) atomicAdd(&bad[W], (int)nb);
    }
}

// the (P label, T label) record of the pair table, or -1 (read-only probing: ln_slot's sequence)
__device__ __forceinline__ long long in_find(const unsigned long long* __restrict__ keys2, unsigned long long cap2, unsigned long long key)
{
    if (cap2 == 0) return -1;
    unsigned long long i = __umul64hi(ln_mix(key), cap2);
    for (unsigned long long t = 0; t < cap2; t++) {
        const unsigned long long k = keys2[i];
        if (k == key) return (long long)i;
        if (k == LN_EMPTY) return -1;
        if (++i == cap2) i = 0;
    }
    return -1;
}

__global__ void k_in_out(long long m, const int* __restrict__ piece, const int* __restrict__ after, const unsigned char* __restrict__ revs,
                         const int* __restrict__ lead, const int* __restrict__ lab, const long long* __restrict__ sh,
                         const int* __restrict__ shbad, int mq, const long long* __restrict__ mir, const int* __restrict__ mirbad,
                         unsigned long long cap2, const unsigned long long* __restrict__ keys2, const long long* __restrict__ pf,
                         const long long* __restrict__ pm, const int* __restrict__ pb, long long* __restrict__ q, const int* __restrict__ bad,
                         unsigned char* __restrict__ st)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int l = lead[k];
    long long v = q[k] + sh[l];
    int b = bad[k] + shbad[l];
    if (mq) {
        const int cp = lab[piece[k]], ct = lab[after[k]];
        const bool rv = revs[k] != 0;
        const long long i = in_find(keys2, cap2, ((unsigned long long)(unsigned)cp << 32) | (unsigned)ct);
        if (i >= 0) {
            v += pf[i];
            if (pb[i] & 1) b++;
            if (rv) { v -= pm[i]; if (pb[i] & 2) b++; }
        }
        if (rv) { v += mir[cp]; b += mirbad[cp]; }
    }
    st[k] = b ? GRAAL_INSERT_NONFINITE : GRAAL_INSERT_VALID;
    q[k] = b ? 0 : v;
}

} // namespace

extern "C" {

int graal_insertions(graal_ctx* h, int32_t max_piece_frags, int64_t* n_out)
{
    if (!h || !n_out) return GRAAL_E_ARG;
    if (max_piece_frags < 1) return fail(h, GRAAL_E_ARG, "graal_insertions: max_piece_frags must be >= 1");
    if (const int rc = score_entry(h, "graal_insertions")) return rc;
    *n_out = 0;
    const int n = h->n, S = h->n_sub_total;
    if (!h->ins) h->ins = new InBuf();
    InBuf* B = h->ins;
    LayoutRecs& R = B->R;
    CandTable& T = B->T;
    B->n_out = -1;
    if (n < 1) { B->n_out = 0; return GRAAL_OK; }
    hipStream_t s = h->stream;
    if (const int rc = recs_reserve(h, R)) return rc;
    CK(group_exact(B->rcap, (size_t)S + 1, B->rowptr, (size_t)S + 1, B->uns, 1));
    const int quirk = (h->mode & GRAAL_MODE_REF_TRANS_ACCU) ? 1 : 0;
    const int mq = quirk && h->n_ubins > 0;
    const int reach = reach_bp(h);
    int rc = GRAAL_OK;
    unsigned err = 0;
    unsigned long long ctr[4] = {0, 0, 0, 0};
    long long m = 0;
    const char* why = nullptr;
    char msg[320];
    do {
        // ---- records (min_frags 1: a record's elig = linear), then the pieces among them
        if ((rc = recs_build(h, R, 1))) break;
        k_in_piece<<<blocks_for(n + 3, 256), 256, 0, s>>>(n + 3, max_piece_frags, R.ctg);
        STEP_CK(hipGetLastError());
        STEP_CK(hipMemsetAsync(B->uns, 0, sizeof(unsigned), s));
        if (h->nnz > 1) {
            k_in_unsorted<<<(unsigned)std::min<long long>(blocks_for(h->nnz, 256), 4096), 256, 0, s>>>(h->row, h->nnz, B->uns);
            STEP_CK(hipGetLastError());
        }
        unsigned uns = 0;
        STEP_CK(hipMemcpyAsync(&err, R.L.err, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(&uns, B->uns, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
        if (err) break;   // (a corrupt layout: the slots and the sub-fragment records are not to be trusted, nothing reads them)
        // ---- row offsets: of the list itself when it is sorted by row, else of its radix sort by row (a permutation, kept for k_in_shift)
        const int* rows = h->row;
        const int* perm = nullptr;
        size_t sort_bytes = 0;
        if (uns) {
            if (h->nnz >= (long long)INT_MAX) {
                snprintf(msg, sizeof msg, "graal_insertions: %lld contacts not sorted by row: upload them sorted", (long long)h->nnz);
                why = msg;
                break;
            }
            const int nz = (int)h->nnz;
            size_t pb = 0;
            STEP_CK(hipcub::DeviceRadixSort::SortPairs(nullptr, pb, (const int*)nullptr, (int*)nullptr, (const int*)nullptr, (int*)nullptr, nz, 0,
                                                     32, s));
            sort_bytes = 3 * sizeof(int) * (size_t)nz + pb;
            if ((size_t)nz > B->pcap || pb > B->ptmp.count)
                STEP_CK(group_realloc(B->pcap, nz, B->srow, nz, B->pin, nz, B->perm, nz, B->ptmp, std::max<size_t>(pb, 1)));
            k_in_iota<<<blocks_for(nz, 256), 256, 0, s>>>(nz, B->pin);
            STEP_CK(hipGetLastError());
            pb = B->ptmp.count;
            STEP_CK(hipcub::DeviceRadixSort::SortPairs(B->ptmp.p, pb, h->row.p, B->srow.p, B->pin.p, B->perm.p, nz, 0, 32, s));
            rows = B->srow;
            perm = B->perm;
        }
        // (a list uploaded sorted by row has the engine's own row index, built at upload: k_rowptr)
        const long long* rowptr = B->rowptr;
        if (!uns && h->rowptr) rowptr = h->rowptr;
        else {
            k_rowptr<<<blocks_for((long long)S + 1, 256), 256, 0, s>>>(S, rows, h->nnz, B->rowptr);
            STEP_CK(hipGetLastError());
        }
        // ---- count pass: upper bounds of the distinct keys of the two tables
        const int nb = stream_blocks(h->nnz);
        if (h->nnz > 0) {
            k_in_nnz<true><<<nb, 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, R.sub, h->stat_frag, R.ctg, R.fr, R.L.slot, h->nfpb, h->par, quirk,
                                              mq, reach, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr,
                                              nullptr, R.ctr, R.L.err);
            STEP_CK(hipGetLastError());
        }
        STEP_CK(hipMemcpyAsync(&err, R.L.err, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(ctr, R.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
        if (err) break;
        const unsigned long long bound = ctr[0];
        const unsigned long long cap = table_cap(bound), cap2 = mq ? table_cap(ctr[3]) : 0;
        const unsigned long long L = bound + 1;
        // device memory: the candidate table (key, q, contacts, flags, selection byte per slot), the (P, T) table (key, far sum, mirror
        // sum, flags), the per-candidate arrays sized to the bound (keys x2, indices x2, q, contacts, T1 x T2 term, bad x2, leader,
        // piece, after, rev, status) and the hipCUB temp storage of the selection, the sort
        unsigned long long need = cap * TABLE_SLOT_BYTES + cap2 * (unsigned long long)(8 + 8 + 8 + 4)
                                  + L * (unsigned long long)(8 * 2 + 4 * 2 + 8 * 3 + 4 * 5 + 1 * 2) + sort_bytes;
        size_t b_sel = 0, b_sort = 0;
        if (cap < (unsigned long long)INT_MAX) {
            STEP_CK(hipcub::DeviceSelect::Flagged(nullptr, b_sel, hipcub::CountingInputIterator<int>(0), (const unsigned char*)nullptr, (int*)nullptr,
                                                (unsigned long long*)nullptr, (int)cap, s));
            STEP_CK(hipcub::DeviceRadixSort::SortPairs(nullptr, b_sort, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                                     (const int*)nullptr, (int*)nullptr, (int)L, 0, 64, s));
        }
        const size_t tneed = std::max(b_sel, b_sort);
        need += tneed;
        if (cap >= (unsigned long long)INT_MAX || cap2 >= (unsigned long long)INT_MAX || need > (unsigned long long)GRAAL_LINKS_MAX_BYTES) {
            snprintf(msg, sizeof msg, "graal_insertions: the candidate table needs %llu bytes (%llu records counted), over the budget of %llu bytes "
                     "(GRAAL_LINKS_MAX_BYTES): use a smaller max_piece_frags", need, ctr[0], (unsigned long long)GRAAL_LINKS_MAX_BYTES);
            why = msg;
            break;
        }
        STEP_CK(table_reserve(T, cap));
        STEP_CK(group_grow(B->cap2, cap2, B->keys2, cap2, B->pf, cap2, B->pm, cap2, B->pb, cap2));
        STEP_CK(group_grow(B->lcap, L, B->ko, L, B->ks, L, B->vo, L, B->vs, L, B->q, L, B->c, L, B->sh, L, B->bad, L, B->shbad, L, B->lead, L,
                           B->piece, L, B->after, L, B->rev, L, B->st, L));
        STEP_CK(scratch_reserve(T, tneed));
        // (the tables are used at sizes `cap` / `cap2`, whatever their allocations: the probe sequences depend on them)
        STEP_CK(table_clear(T, cap, s));
        if (cap2) {
            STEP_CK(hipMemsetAsync(B->keys2, 0xff, sizeof(unsigned long long) * cap2, s));
            STEP_CK(hipMemsetAsync(B->pf, 0, sizeof(long long) * cap2, s));
            STEP_CK(hipMemsetAsync(B->pm, 0, sizeof(long long) * cap2, s));
            STEP_CK(hipMemsetAsync(B->pb, 0, sizeof(int) * cap2, s));
        }
        // ---- insert pass, selection of the listed slots, sort by key
        if (h->nnz > 0) {
            k_in_nnz<false><<<nb, 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, R.sub, h->stat_frag, R.ctg, R.fr, R.L.slot, h->nfpb, h->par, quirk,
                                               mq, reach, cap, T.keys, T.tq, T.tc, T.tf, cap2, B->keys2, B->pf, B->pm, B->pb, R.mir,
                                               R.mirbad, R.ctr, R.L.err);
            STEP_CK(hipGetLastError());
        }
        k_ln_flag<<<blocks_for((long long)cap, 256), 256, 0, s>>>(T.keys, T.tf, (long long)cap, T.tsel);
        STEP_CK(hipGetLastError());
        size_t tb = T.stmp.count;
        STEP_CK(hipcub::DeviceSelect::Flagged(T.stmp, tb, hipcub::CountingInputIterator<int>(0), (const unsigned char*)T.tsel, B->vo.p, &R.ctr[1],
                                            (int)cap, s));
        STEP_CK(hipMemcpyAsync(ctr, R.ctr, sizeof(ctr), hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(&err, R.L.err, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
        if (err) break;
        m = (long long)ctr[1];
        if (m == 0) break;
        if ((m + 3) / 4 > (long long)INT_MAX) {
            snprintf(msg, sizeof msg, "graal_insertions: %lld candidates exceed one launch: use a smaller max_piece_frags", m);
            why = msg;
            break;
        }
        k_ln_keys<<<blocks_for(m, 256), 256, 0, s>>>(m, T.keys, B->vo, B->ko);
        STEP_CK(hipGetLastError());
        tb = T.stmp.count;
        STEP_CK(hipcub::DeviceRadixSort::SortPairs(T.stmp.p, tb, B->ko.p, B->ks.p, B->vo.p, B->vs.p, (int)m, 0, 64, s));
        k_in_gather<<<blocks_for(m, 256), 256, 0, s>>>(m, B->ks, B->vs, T.tq, T.tc, T.tf, B->q, B->c, B->bad, B->sh, B->shbad, B->piece,
                                                       B->after, B->rev);
        STEP_CK(hipGetLastError());
        k_in_lead<<<blocks_for(m, 256), 256, 0, s>>>(m, B->piece, B->after, R.lab, R.ctg, B->lead);
        STEP_CK(hipGetLastError());
        // ---- the mass passes, the quirk's passes, the result
        const unsigned wblocks = (unsigned)((m + 3) / 4);            // a wave per candidate, 4 waves per block
        k_in_mass<<<wblocks, 256, 0, s>>>(m, B->piece, B->after, B->rev, R.L.slot, R.lab, R.ctg, R.fr, h->nfpb, h->par, quirk, reach, B->q,
                                          B->bad);
        STEP_CK(hipGetLastError());
        k_in_shift<<<wblocks, 256, 0, s>>>(m, B->lead, B->piece, B->after, R.L.slot, R.lab, R.ctg, R.fr, R.sub, h->stat_frag, h->d_sub_ids,
                                           rowptr, perm, h->col, h->cnt, h->nfpb, h->par, reach, B->sh, B->shbad);
        STEP_CK(hipGetLastError());
        if (mq) {
            k_ln_mirror<<<h->n_ubins, 256, 0, s>>>(n, h->d_ubins, R.L.slot, R.lab, R.ctg, R.fr, h->nfpb, h->par, R.mir, R.mirbad);
            STEP_CK(hipGetLastError());
            k_in_quirk<<<wblocks, 256, 0, s>>>(m, B->piece, B->after, B->rev, R.L.slot, R.lab, R.ctg, R.fr, h->nfpb, h->par, reach, B->q, B->bad);
            STEP_CK(hipGetLastError());
        }
        k_in_out<<<blocks_for(m, 256), 256, 0, s>>>(m, B->piece, B->after, B->rev, B->lead, R.lab, B->sh, B->shbad, mq, R.mir, R.mirbad, cap2,
                                                    B->keys2, B->pf, B->pm, B->pb, B->q, B->bad, B->st);
        STEP_CK(hipGetLastError());
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    if (const int r = score_exit(h, "graal_insertions", rc, why, err)) return r;
    B->n_out = m;
    *n_out = m;
    return GRAAL_OK;
}

int graal_insertions_fetch(graal_ctx* h, int32_t* piece, int32_t* after, uint8_t* rev, int64_t* q, int64_t* contacts, uint8_t* status, int64_t cap)
{
    if (!h || !piece || !after || !rev || !q || !contacts || !status) return GRAAL_E_ARG;
    InBuf* B = h->ins;
    if (!B || B->n_out < 0) return fail(h, GRAAL_E_STATE, "graal_insertions_fetch: call graal_insertions first");
    const long long m = B->n_out;
    if (cap < m) return fail(h, GRAAL_E_ARG, "graal_insertions_fetch: cap is smaller than the number of candidates");
    if (m == 0) return GRAAL_OK;
    CK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    CK(hipMemcpyAsync(piece, B->piece, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(after, B->after, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(rev, B->rev, (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(q, B->q, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(contacts, B->c, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(status, B->st, (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    return GRAAL_OK;
}

} // extern "C"
