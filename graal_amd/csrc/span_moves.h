// span_moves.h -- the likelihood each move of a span of fragments would add, for a caller's set of disjoint spans in one pass: in-place
// reversals (graal_block_flips) and swaps of two adjacent runs (graal_block_swaps); and the frame of every call that scores spans
// (span_moves: these two and excise.h's graal_block_excisions).  Included by graal_hip.hip after insert.h (it uses LayoutRecs with
// recs_reserve / recs_build, slots_read_err, the records LnFrag / LnCtg, ln_block_add, ln_mirror_q, span_check.h, wave_runs.h's run_sums
// and score_common.h's score_entry, score_exit, STEP_CK and stream_blocks).
//
// Span k = the fragments of one linear contig at slots first .. last, bp interval [s0, e1).  The breakpoint sm behind slot mid splits it
// into the runs X = first .. mid and Y = mid + 1 .. last (lx = sm - s0, ly = e1 - sm).  The moved layout puts Y in front of X:
// Y' = [s0, s0 + ly), X' = [s0 + ly, e1); the bit `rev` of the call says whether X is reversed inside X'.  A fragment (start, len) of a
// run that occupies [lo, hi) now and [lo', hi') afterwards goes to lo' + (start - lo), or reversed to hi' - (start - lo + len) with its
// ori toggled; every other field stays; the float32 centres through centre_kb from the new integer starts.
//   a flip:  mid = last, sm = e1, rev = 1.  Y is empty, X' = X: the block is reversed inside its interval.
//   a swap:  rev = 0.  A fragment of X moves ly bp up, a fragment of Y lx bp down, nothing is turned round.
// M(k) = logL(moved) - logL(current) in the exact arithmetic with the roundings of junctions.h / links.h: pairs inside X, inside Y and
// outside the span count as unchanged; every sub-fragment pair of X x Y, X x rest and Y x rest (rest: the contig's other fragments) moves
// from its cis price to its cis price in the moved layout
//   a contact:                ob * (ln ex_new - ln ex_old), rounded to Q once per contact (0 where the two prices are the same float32);
//   a fragment pair's mass:   -(sum over its sub-fragment pairs of ex_new - ex_old), the moved run's fragment outer (X's for X x Y),
//                             rounded to Q once.
// The window.  A fragment x of the span lies L0 = start - s0 behind the span's left boundary and R0 = e1 - (start + len) before its right
// one, L1 and R1 in the moved layout; a flank fragment y lies g bp outside the boundary it faces.  The pair is beyond the window both
// times -- priced v_inter * norm twice, difference exactly 0 -- unless min(L0, L1) + g <= reach_bp (left flank) or min(R0, R1) + g <=
// reach_bp (right flank).  For a flip L1 = R0 and R1 = L0: both budgets are reach_bp - min(L0, R0).  For a swap, with dl / dr the distance
// of x to its own run's left / right end, the pair's gap is, before and after,
//   x in X, left flank:  dl + g        and dl + ly + g        x in X, right flank: dr + ly + g  and dr + g
//   x in Y, left flank:  dl + lx + g   and dl + g             x in Y, right flank: dr + g       and dr + lx + g
//   x in X, y in Y:      dr(x) + dl(y) and dl(x) + dr(y)
// so only the run fragments within reach of one of their run's ends, and partners within reach of a boundary or the breakpoint, take
// part: at most about (2w) x (2w) fragment pairs per flip and (4w) x (3w) per swap, however long the runs.
// Under GRAAL_MODE_REF_TRANS_ACCU a reversed run changes the orientation of its bins of mixed RF counts, and with it the trans price of
// every pair (such a bin x, a higher-id bin y of ANOTHER contig): links.h's mirror term, summed per span.  Cis prices do not use the
// indexing, so nothing else changes inside the contig, and a call with rev = 0 does not depend on the mode.
//
// Every fragment belongs to at most one span, so a contact feeds at most two sums and the list is streamed once; no candidate table.
// Kernels, all on the engine's stream:
//   k_jn_count / scan / k_ln_prep (recs_build) -- slots and per-slot records, as for links and insertions;
//   k_sp_gather -- per span of the caller: the slots and labels of its fragments, its bp interval and breakpoint, its contig's slots.  The
//                 host decides from these (span_check.h): refuses the call, or sets aside the spans in a ring (and, for flips, those
//                 that are a whole contig) and uploads the others sorted by first slot;
//   k_sp_sub    -- per fragment: its span (binary search over the sorted spans), its run and, per sub-fragment, a 32-byte record with its
//                 current and its moved centre (well defined: a fragment belongs to at most one span);
//   k_sp_nnz    -- streams the contact list once, 64 consecutive contacts per wave.  A contact of one contig is priced when its sides
//                 differ in (span, run): once for the span with both sides moved when they are its X and its Y, else once per side that
//                 has a span, with that side moved alone.  Sums per run of equal span inside the wave (run_sums) before the atomics;
//                 the mirror's contact part rides along;
//   k_sp_edges / scan / k_sp_mass -- work units (span, one fragment of X or Y within reach of an end of its run) from a prefix sum, a wave
//                 per unit; its lanes walk the partner ranges outwards from the boundaries 64 fragments at a time (each partner record is
//                 read once, by one lane: nothing to stage) and stop when a whole step is out of reach; one atomic per wave;
//   k_sp_mirror -- only for a reversing call with the mode flag and mixed bins: one workgroup per mixed bin, links' per-bin term;
//   k_sp_out    -- status and q per span, in the caller's order.
#pragma once

#include "span_check.h"

namespace {

// acc: RF count | the bin's last RF count << 16; meta: fwd | mixed << 1 | reversed by the move << 2 | in Y << 3
struct SpanSub { float c_old, c_new; int label, span, frag, acc, meta, pad; };
constexpr size_t SPAN_SUB_BYTES = 32;                                 // of every kind's record: they share SpanBuf's allocation, sized by S
static_assert(sizeof(SpanSub) == SPAN_SUB_BYTES, "a sub-fragment's record is two 16-byte loads");

// One set per handle for the three calls: each call rebuilds what it reads.
struct SpanBuf {
    LayoutRecs R;
    DevBuf<SpanSub> sub; int n = 0, S = 0;                            // per sub-fragment: a SpanSub, or excise.h's ExSub (32 bytes each)
    DevBuf<int> first, mid, last; DevBuf<SpanInfo> info; DevBuf<SpanRec> rec;
    DevBuf<long long> qb, cb, q, c, ne, noff; DevBuf<int> bad; DevBuf<int4> nx;
    DevBuf<unsigned char> st;
    DevBuf<void> tmp;
    size_t bcap = 0;                                                  // spans the per-span arrays hold
};

void sp_free(SpanBuf* b) { delete b; }

// mid: null for a call without a breakpoint (mid = last)
__global__ void k_sp_gather(int nb, int n, const int* __restrict__ first, const int* __restrict__ mid, const int* __restrict__ last,
                            const int* __restrict__ slot_of, const int* __restrict__ lab, const LnFrag* __restrict__ fr,
                            const LnCtg* __restrict__ ctg, SpanInfo* __restrict__ info)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    SpanInfo r = {-1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0};
    const int f = first[k], l = last[k], m = mid ? mid[k] : l;       // (in [0, n): the host checked)
    const int sf = slot_of[f], sm = slot_of[m], sl = slot_of[l];
    if (sf >= 0 && sf < n && sm >= 0 && sm < n && sl >= 0 && sl < n) {
        r.slot_f = sf; r.slot_m = sm; r.slot_l = sl; r.lab_f = lab[f]; r.lab_m = lab[m]; r.lab_l = lab[l];
        const LnFrag a = fr[sf], x = fr[sm], b = fr[sl];
        r.s0 = a.start; r.sm = x.start + x.len; r.e1 = b.start + b.len;
        const LnCtg c = ctg[r.lab_f];
        r.cfirst = c.first; r.ccnt = c.cnt; r.circ = c.elig ? 0 : 1;   // (records built with min_frags 1: elig = linear)
    }
    info[k] = r;
}

// the scored span that holds `slot`, or -1: the last span that starts at or before it, if it reaches that far.  ub: the number of
// scored spans that start at or before the slot
__device__ __forceinline__ int sp_span_of(const SpanRec* __restrict__ rec, int m, int slot, int* ub = nullptr)
{
    int lo = 0, hi = m;                                              // first span with .first > slot
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rec[mid].first <= slot) lo = mid + 1; else hi = mid;
    }
    if (ub) *ub = lo;
    return (lo > 0 && slot <= rec[lo - 1].last) ? lo - 1 : -1;
}

// where the move puts a fragment (start, len) of span b's run X (in_y false) or Y; turned: X is reversed inside its new interval
__device__ __forceinline__ int sp_new_start(const SpanRec& b, bool in_y, bool turned, int start, int len)
{
    const long long ly = (long long)b.e1 - b.sm;
    if (in_y) return (int)((long long)b.s0 + ((long long)start - b.sm));
    if (turned) return (int)((long long)b.e1 - ((long long)start - b.s0 + len));   // (the sum of two offsets may pass 2^31)
    return (int)((long long)b.s0 + ly + ((long long)start - b.s0));
}

__global__ __launch_bounds__(256) void k_sp_sub(int n, int m, int rev, const SpanRec* __restrict__ rec, const int* __restrict__ slot_of,
                                                const int* __restrict__ lab, const LnFrag* __restrict__ fr, const int* __restrict__ sub_ids,
                                                SpanSub* __restrict__ sub)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int slot = slot_of[f];
    if (slot < 0 || slot >= n) return;                               // (a corrupt layout: refused before anything reads the records)
    const LnFrag x = fr[slot];
    const int j = sp_span_of(rec, m, slot);
    int ns = x.start;
    bool in_y = false, turned = false;
    if (j >= 0) {
        const SpanRec b = rec[j];
        in_y = slot > b.mid; turned = rev && !in_y;
        ns = sp_new_start(b, in_y, turned, x.start, x.len);
    }
    const bool fo = x.fwd != 0;
    const int last = stat_accu(x.st, x.st.n - 1);
    int4 ids = make_int4(f, 0, 0, 1);
    if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[f];
    for (int k = 0; k < x.st.n; k++) {
        SpanSub u;
        u.c_old = centre_kb(x.start, fo, x.st, k);
        u.c_new = j >= 0 ? centre_kb(ns, fo != turned, x.st, k) : u.c_old;
        u.label = lab[f]; u.span = j; u.frag = f; u.pad = 0;
        u.acc = stat_accu(x.st, k) | (last << 16);                   // (RF counts are <= 30000)
        u.meta = (fo ? 1 : 0) | (stat_uniform(x.st) ? 0 : 2) | (turned ? 4 : 0) | (in_y ? 8 : 0);
        sub[sel3(ids.x, ids.y, ids.z, k)] = u;
    }
}

// a contact of a span's sub-fragment whose centre the move takes to distance sd_new from its partner: the term, the count inside the window
__device__ __forceinline__ void sp_contact(float sd_new, float ex_old, float norm, double ob, const Par& par, long long& q, long long& c, long long& bad)
{
    if (sd_new < par.d_max) c = (long long)llrint(ob);
    const float ex_new = rippe(sd_new, par) * norm;
    if (ex_new == ex_old) return;                                    // (both beyond the window, or the distance did not change)
    const long long t = to_q(ob * (mm_ln(ex_new) - mm_ln(ex_old)));
    if (t == Q_BAD) bad = 1; else q = t;
}

__device__ __forceinline__ void sp_add(unsigned long long key, long long q, long long c, long long bad, long long* __restrict__ qb,
                                       long long* __restrict__ cb, int* __restrict__ badb)
{
    bool tail;
    run_sums(key, tail, q, c, bad);
    if (tail && key != LN_EMPTY) {
        if (q != 0) atomicAdd((unsigned long long*)&qb[key], (unsigned long long)q);
        if (c != 0) atomicAdd((unsigned long long*)&cb[key], (unsigned long long)c);
        if (bad != 0) atomicAdd(&badb[key], (int)bad);
    }
}

// mirror: the mode flag of a reversing call
__global__ __launch_bounds__(256) void k_sp_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt, long long nnz,
                                                const SpanSub* __restrict__ sub, float nfpb, Par par, int mirror, long long* __restrict__ qb,
                                                long long* __restrict__ cb, int* __restrict__ badb)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {   // (wave-uniform bounds: the run sums need the whole wave)
        const long long k = k0 + lane;
        unsigned long long ka = LN_EMPTY, kb = LN_EMPTY;
        long long qa = 0, ca = 0, ba = 0, qc = 0, cc = 0, bc = 0;
        if (k < nnz) {
            const SpanSub A = sub[row[k]], B = sub[col[k]];
            const double ob = (double)__int_as_float(cnt[k]);
            const int own_a = A.acc & 0xffff, own_b = B.acc & 0xffff;
            if (A.label == B.label) {
                if (A.span != B.span || ((A.meta ^ B.meta) & 8)) {   // (sub-fragments of one bin share span and run)
                    const float norm = (float)(own_a * own_b) / nfpb;
                    const float ex_old = rippe(fabsf(B.c_old - A.c_old), par) * norm;
                    if (A.span == B.span) { ka = (unsigned long long)A.span; sp_contact(fabsf(B.c_new - A.c_new), ex_old, norm, ob, par, qa, ca, ba); }
                    else {
                        if (A.span >= 0) { ka = (unsigned long long)A.span; sp_contact(fabsf(B.c_old - A.c_new), ex_old, norm, ob, par, qa, ca, ba); }
                        if (B.span >= 0) { kb = (unsigned long long)B.span; sp_contact(fabsf(B.c_new - A.c_old), ex_old, norm, ob, par, qc, cc, bc); }
                    }
                }
            } else if (mirror) {                                     // the mirror's contact part: the lower-id bin's orientation picks the indexing
                const bool a_low = A.frag < B.frag;
                const SpanSub& lo = a_low ? A : B;
                if ((lo.meta & 6) == 6) {                            // (a mixed bin that the move turns round)
                    const int own_l = lo.acc & 0xffff, last_l = lo.acc >> 16, other = a_low ? own_b : own_a;
                    const bool fwd = lo.meta & 1;
                    const int prod_t = (fwd ? own_l : last_l) * other, prod_f = (fwd ? last_l : own_l) * other;
                    if (prod_f != prod_t) {
                        const float et = par.v_inter * ((float)prod_t / nfpb), ef = par.v_inter * ((float)prod_f / nfpb);
                        const long long t = to_q(ob * (mm_ln(ef) - mm_ln(et)));
                        if (a_low) { ka = (unsigned long long)A.span; if (t == Q_BAD) ba = 1; else qa = t; }
                        else { kb = (unsigned long long)B.span; if (t == Q_BAD) bc = 1; else qc = t; }
                    }
                }
            }
        }
        if (__ballot(ka != LN_EMPTY) != 0ull) sp_add(ka, qa, ca, ba, qb, cb, badb);
        if (__ballot(kb != LN_EMPTY) != 0ull) sp_add(kb, qc, cc, bc, qb, cb, badb);
    }
}

// the fragments of the run of slots [a, b] in the bp interval [lo_bp, hi_bp) within reach of an end: (units, those counted from the left);
// all of them when the two groups meet, (0, 0) for an empty run.  Starts grow with the slot, so both counts come from binary searches.
__device__ __forceinline__ int2 sp_run_edges(const LnFrag* __restrict__ fr, int a, int b, int lo_bp, int hi_bp, int reach_bp)
{
    const int len = b - a + 1;
    int lo = 0, hi = len;                                            // first u with dl > reach
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)fr[a + mid].start - lo_bp <= reach_bp) lo = mid + 1; else hi = mid;
    }
    const int n_left = lo;
    lo = 0; hi = len;                                                // first u (counted from the last slot down) with dr > reach
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const LnFrag x = fr[b - mid];
        if ((long long)hi_bp - ((long long)x.start + x.len) <= reach_bp) lo = mid + 1; else hi = mid;
    }
    const int n_right = lo;
    if ((long long)n_left + n_right >= len) return make_int2(len, len);
    return make_int2(n_left + n_right, n_left);
}

// per span: the units of X and of Y (nx = units of X, of them from the left, units of Y, of them from the left); ne = their sum
__global__ void k_sp_edges(int m, const SpanRec* __restrict__ rec, const LnFrag* __restrict__ fr, int reach_bp, long long* __restrict__ ne,
                           int4* __restrict__ nx)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > m) return;
    if (j == m) { ne[m] = 0; return; }                               // (the scan's last entry: the total)
    const SpanRec b = rec[j];
    const int2 x = sp_run_edges(fr, b.first, b.mid, b.s0, b.sm, reach_bp), y = sp_run_edges(fr, b.mid + 1, b.last, b.sm, b.e1, reach_bp);
    ne[j] = x.x + y.x;
    nx[j] = make_int4(x.x, x.y, y.x, y.y);
}

// mass term of the moved fragment x (current centres xo, moved centres xn) and a partner y that sits at y.start now and at ys_new in the
// moved layout: -(sum of ex_new - ex_old), x outer
__device__ __forceinline__ long long sp_pair_q(const LnFrag& x, float xo0, float xo1, float xo2, float xn0, float xn1, float xn2, const LnFrag& y,
                                               int ys_new, float nfpb, const Par& par)
{
    double acc = 0.0;
    for (int a = 0; a < x.st.n; a++) {
        const int ax = stat_accu(x.st, a);
        const float co = sel3(xo0, xo1, xo2, a), cn = sel3(xn0, xn1, xn2, a);
        for (int b = 0; b < y.st.n; b++) {
            const float norm = (float)(ax * stat_accu(y.st, b)) / nfpb;
            const float yo = centre_kb(y.start, y.fwd != 0, y.st, b);
            const float yn = ys_new == y.start ? yo : centre_kb(ys_new, y.fwd != 0, y.st, b);
            acc += ((double)(rippe(fabsf(yn - cn), par) * norm) - (double)(rippe(fabsf(yo - co), par) * norm));   // (new - old is exact in float64)
        }
    }
    return to_q_fast(acc);
}

// the unit's span: the last j with noff[j] <= W (every scored span has at least one unit: a fragment of X)
__device__ __forceinline__ int sp_span_of_unit(const long long* __restrict__ noff, int m, long long W)
{
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (noff[mid] <= W) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One walk of a unit: partners from slot `from` in steps of `dir` while inside [lo_slot, hi_slot], the partner's gap to the boundary
// `edge` it is walked away from must be <= budget (the gap only grows); a partner whose gap to `skip_edge` on its other side is <=
// skip_budget was priced by an earlier walk (X x Y only; skip_budget < 0: none).  shift: what the move adds to the partner's start.
__device__ __forceinline__ void sp_walk(const LnFrag* __restrict__ fr, int from, int dir, int lo_slot, int hi_slot, int edge, long long budget,
                                        int skip_edge, long long skip_budget, int shift, const LnFrag& x, float xo0, float xo1, float xo2,
                                        float xn0, float xn1, float xn2, float nfpb, const Par& par, long long& sum, long long& nb)
{
    if (budget < 0) return;                                          // (wave-uniform)
    const int lane = threadIdx.x & 63;
    for (long long t = lane; ; t += 64) {
        const long long i = (long long)from + dir * t;
        bool in = i >= lo_slot && i <= hi_slot;
        bool take = false;
        LnFrag y;
        if (in) {
            y = fr[i];
            const long long g = dir < 0 ? (long long)edge - ((long long)y.start + y.len) : (long long)y.start - edge;
            in = g <= budget;
            take = in;
            if (in && skip_budget >= 0) {
                const long long g2 = dir < 0 ? (long long)y.start - skip_edge : (long long)skip_edge - ((long long)y.start + y.len);
                take = g2 > skip_budget;
            }
        }
        if (__ballot(in) == 0ull) break;
        if (take) {
            const long long q = sp_pair_q(x, xo0, xo1, xo2, xn0, xn1, xn2, y, y.start + shift, nfpb, par);
            if (q == Q_BAD) nb++; else sum -= q;
        }
    }
}

__global__ __launch_bounds__(256) void k_sp_mass(long long total, int m, int rev, const SpanRec* __restrict__ rec,
                                                 const long long* __restrict__ noff, const long long* __restrict__ ne,
                                                 const int4* __restrict__ nx, const LnFrag* __restrict__ fr, float nfpb, Par par, int reach_bp,
                                                 long long* __restrict__ qb, int* __restrict__ badb)
{
    const long long W = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (W >= total) return;                                          // (wave-uniform)
    const int j = sp_span_of_unit(noff, m, W);
    if (W - noff[j] < 0 || W - noff[j] >= ne[j]) return;
    int u = (int)(W - noff[j]);                                      // (< the span's fragments)
    const SpanRec b = rec[j];
    const int4 e = nx[j];
    const bool in_y = u >= e.x;
    if (in_y) u -= e.x;
    const int left = in_y ? e.w : e.y;
    const int ra = in_y ? b.mid + 1 : b.first, rb = in_y ? b.last : b.mid;   // the unit's run
    const int slot = u < left ? ra + u : rb - (u - left);
    if (slot < ra || slot > rb) return;
    const LnFrag x = fr[slot];
    const bool turned = rev && !in_y;
    const int ns = sp_new_start(b, in_y, turned, x.start, x.len);
    const bool fo = x.fwd != 0, fn = fo != turned;
    const float xo0 = centre_kb(x.start, fo, x.st, 0), xo1 = x.st.n > 1 ? centre_kb(x.start, fo, x.st, 1) : 0.0f,
                xo2 = x.st.n > 2 ? centre_kb(x.start, fo, x.st, 2) : 0.0f;
    const float xn0 = centre_kb(ns, fn, x.st, 0), xn1 = x.st.n > 1 ? centre_kb(ns, fn, x.st, 1) : 0.0f,
                xn2 = x.st.n > 2 ? centre_kb(ns, fn, x.st, 2) : 0.0f;
    long long sum = 0, nb = 0;
    // the flanks: a partner at gap g takes part while the smaller of x's two distances to the boundary it faces, now and moved, + g <= reach
    const long long l0 = (long long)x.start - b.s0, r0 = (long long)b.e1 - ((long long)x.start + x.len);
    const long long l1 = (long long)ns - b.s0, r1 = (long long)b.e1 - ((long long)ns + x.len);
    sp_walk(fr, b.first - 1, -1, b.cfirst, b.first - 1, b.s0, reach_bp - min(l0, l1), 0, -1, 0, x, xo0, xo1, xo2, xn0, xn1, xn2, nfpb, par, sum, nb);
    sp_walk(fr, b.last + 1, 1, b.last + 1, b.clast, b.e1, reach_bp - min(r0, r1), 0, -1, 0, x, xo0, xo1, xo2, xn0, xn1, xn2, nfpb, par, sum, nb);
    if (!in_y && b.mid < b.last) {
        // X x Y (X not turned: no caller moves a reversed X past a Y): now the gap is dr(x) + dl(y), walked from Y's left end; moved it is
        // dl(x) + dr(y), walked from Y's right end, less the pairs the first walk took
        const int lx = b.sm - b.s0;
        const long long dr = (long long)b.sm - ((long long)x.start + x.len);
        sp_walk(fr, b.mid + 1, 1, b.mid + 1, b.last, b.sm, reach_bp - dr, 0, -1, -lx, x, xo0, xo1, xo2, xn0, xn1, xn2, nfpb, par, sum, nb);
        sp_walk(fr, b.last, -1, b.mid + 1, b.last, b.e1, reach_bp - l0, b.sm, reach_bp - dr, -lx, x, xo0, xo1, xo2, xn0, xn1, xn2, nfpb, par, sum, nb);
    }
    ln_block_add(sum, nb, &qb[j], &badb[j]);
}

// the mirror's mass part: one workgroup per mixed bin x of a scored span's reversed run, against every higher-id bin of another contig
// (k_ln_mirror's term)
__global__ __launch_bounds__(256) void k_sp_mirror(int n, int m, const SpanRec* __restrict__ rec, const int* __restrict__ ubins,
                                                   const int* __restrict__ slot_of, const int* __restrict__ lab, const LnFrag* __restrict__ fr,
                                                   float nfpb, Par par, long long* __restrict__ qb, int* __restrict__ badb)
{
    const int xf = ubins[blockIdx.x];
    if (xf < 0 || xf >= n) return;
    const int sx = slot_of[xf];
    if (sx < 0 || sx >= n) return;
    const int j = sp_span_of(rec, m, sx);
    if (j < 0 || sx > rec[j].mid) return;
    const int c = lab[xf];
    const LnFrag x = fr[sx];
    if (x.st.n < 1) return;
    long long sum = 0, nb = 0;
    for (int y = xf + 1 + (int)threadIdx.x; y < n; y += (int)blockDim.x) {
        const int sy = slot_of[y];
        if (lab[y] == c || sy < 0 || sy >= n) continue;
        const long long t = ln_mirror_q(x, fr[sy], nfpb, par);
        if (t == Q_BAD) nb++; else sum += t;
    }
    ln_block_add(sum, nb, &qb[j], &badb[j]);
}

__global__ void k_sp_out(int m, const SpanRec* __restrict__ rec, const long long* __restrict__ qb, const long long* __restrict__ cb,
                         const int* __restrict__ badb, unsigned char valid, unsigned char nonfinite, long long* __restrict__ q,
                         long long* __restrict__ c, unsigned char* __restrict__ st)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int id = rec[j].id;
    const bool bad = badb[j] != 0;
    st[id] = bad ? nonfinite : valid;
    q[id] = bad ? 0 : qb[j];
    c[id] = cb[j];
}

// The units' total behind a kind's edges kernel: the exclusive scan of ne over m + 1 entries, read back (a host wait).
int sp_unit_total(graal_ctx* h, SpanBuf* B, int m, long long& total)
{
    hipStream_t s = h->stream;
    int rc = GRAAL_OK;
    do {
        size_t tb = B->tmp.count;
        STEP_CK(hipcub::DeviceScan::ExclusiveSum(B->tmp.p, tb, B->ne.p, B->noff.p, m + 1, s));
        STEP_CK(hipMemcpyAsync(&total, B->noff + m, sizeof(long long), hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    return rc;
}

// The kernels of a flip or a swap: what span_moves runs between the upload of the m scored spans and k_sp_out.
int sp_score(graal_ctx* h, const SpanKind& K, SpanBuf* B, const std::vector<SpanRec>& rec, std::string&)
{
    const int n = h->n, m = (int)rec.size();
    const LayoutRecs& R = B->R;
    SpanSub* const sub = (SpanSub*)B->sub;
    hipStream_t s = h->stream;
    const int mirror = (K.rev && (h->mode & GRAAL_MODE_REF_TRANS_ACCU)) ? 1 : 0;
    int rc = GRAAL_OK;
    do {
        k_sp_sub<<<blocks_for(n, 256), 256, 0, s>>>(n, m, K.rev, B->rec, R.L.slot, R.lab, R.fr, h->d_sub_ids, sub);
        STEP_CK(hipGetLastError());
        if (h->nnz > 0) {
            k_sp_nnz<<<stream_blocks(h->nnz), 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, sub, h->nfpb, h->par, mirror, B->qb, B->cb, B->bad);
            STEP_CK(hipGetLastError());
        }
        k_sp_edges<<<blocks_for(m + 1, 256), 256, 0, s>>>(m, B->rec, R.fr, reach_bp(h), B->ne, B->nx);
        STEP_CK(hipGetLastError());
        long long total = 0;                                          // (<= n: a fragment belongs to at most one span)
        if ((rc = sp_unit_total(h, B, m, total))) break;
        if (total > 0) {
            k_sp_mass<<<blocks_for(total, 4), 256, 0, s>>>(total, m, K.rev, B->rec, B->noff, B->ne, B->nx, R.fr, h->nfpb, h->par, reach_bp(h), B->qb, B->bad);
            STEP_CK(hipGetLastError());
        }
        if (mirror && h->n_ubins) {
            k_sp_mirror<<<h->n_ubins, 256, 0, s>>>(n, m, B->rec, h->d_ubins, R.L.slot, R.lab, R.fr, h->nfpb, h->par, B->qb, B->bad);
            STEP_CK(hipGetLastError());
        }
    } while (false);
    return rc;
}

// The frame of the three calls.  mid: null for a kind without one.  kernels: the kind's kernels over the scored spans
// `rec` (at least one; uploaded to B->rec, the sums qb / cb / bad cleared), which leave the sums for k_sp_out; it returns a scorer's rc
// and may set `unsupported`, the text of a call it cannot serve.  kernels(h, K, B, rec, unsupported).
template <class Kernels>
int span_moves(graal_ctx* h, const SpanKind& K, int nb, const int32_t* first, const int32_t* mid, const int32_t* last, int64_t* q,
               int64_t* contacts, uint8_t* status, Kernels kernels)
{
    if (const int rc = score_entry(h, K.fn)) return rc;
    if (nb == 0) return GRAAL_OK;
    const int n = h->n, S = h->n_sub_total;
    char msg[240], why[64];
    for (int k = 0; k < nb; k++)
        if (first[k] < 0 || first[k] >= n || last[k] < 0 || last[k] >= n || (mid && (mid[k] < 0 || mid[k] >= n))) {
            if (mid) snprintf(msg, sizeof msg, "%s: %s %d: fragment index out of range (%d, %d, %d; %d fragments)", K.fn, K.noun, k, first[k], mid[k], last[k], n);
            else snprintf(msg, sizeof msg, "%s: %s %d: fragment index out of range (%d, %d; %d fragments)", K.fn, K.noun, k, first[k], last[k], n);
            return fail(h, GRAAL_E_ARG, msg);
        }
    if (!h->sp) h->sp = new SpanBuf();
    SpanBuf* B = h->sp;
    LayoutRecs& R = B->R;
    hipStream_t s = h->stream;
    if (const int rc = recs_reserve(h, R)) return rc;
    if (B->n != n || B->S != S) {
        CK(group_realloc(B->n, n, B->sub, std::max(S, 1)));
        B->S = S;
    }
    if ((size_t)nb > B->bcap) {                                       // (grows to the largest call of any kind)
        const size_t cap = (size_t)nb + 1;
        size_t tb = 0;
        CK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (long long*)nullptr, (long long*)nullptr, (int)cap, s));
        CK(group_realloc(B->bcap, nb, B->first, cap, B->mid, cap, B->last, cap, B->bad, cap, B->qb, cap, B->cb, cap, B->q, cap, B->c, cap, B->ne, cap,
                         B->noff, cap, B->info, cap, B->rec, cap, B->nx, cap, B->st, cap, B->tmp, tb));
    }
    int rc = GRAAL_OK;
    unsigned err = 0;
    bool refused = false;
    std::string unsupported;
    std::vector<SpanInfo> info((size_t)nb);
    do {
        if ((rc = recs_build(h, R, 1))) break;
        STEP_CK(hipMemcpyAsync(B->first, first, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, s));
        if (mid) STEP_CK(hipMemcpyAsync(B->mid, mid, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, s));
        STEP_CK(hipMemcpyAsync(B->last, last, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, s));
        k_sp_gather<<<blocks_for(nb, 256), 256, 0, s>>>(nb, n, B->first, mid ? B->mid.p : nullptr, B->last, R.L.slot, R.lab, R.fr, R.ctg, B->info);
        STEP_CK(hipGetLastError());
        STEP_CK(hipMemcpyAsync(info.data(), B->info, sizeof(SpanInfo) * (size_t)nb, hipMemcpyDeviceToHost, s));
        if ((rc = slots_read_err(h, R.L, err)) || err) break;
        const SpanChecked C = span_check(info.data(), nb, K);
        if (C.off >= 0) {
            span_reason_text(K, C.why, why, sizeof why);
            if (mid) snprintf(msg, sizeof msg, "%s: %s %d (fragments %d .. %d .. %d): %s", K.fn, K.noun, C.off, first[C.off], mid[C.off], last[C.off], why);
            else snprintf(msg, sizeof msg, "%s: %s %d (fragments %d .. %d): %s", K.fn, K.noun, C.off, first[C.off], last[C.off], why);
            refused = true;
            break;
        }
        const int m = (int)C.rec.size();
        STEP_CK(hipMemsetAsync(B->q, 0, sizeof(long long) * (size_t)nb, s));
        STEP_CK(hipMemsetAsync(B->c, 0, sizeof(long long) * (size_t)nb, s));
        STEP_CK(hipMemcpyAsync(B->st, C.st.data(), (size_t)nb, hipMemcpyHostToDevice, s));
        if (m > 0) {
            STEP_CK(hipMemcpyAsync(B->rec, C.rec.data(), sizeof(SpanRec) * (size_t)m, hipMemcpyHostToDevice, s));
            STEP_CK(hipMemsetAsync(B->qb, 0, sizeof(long long) * (size_t)m, s));
            STEP_CK(hipMemsetAsync(B->cb, 0, sizeof(long long) * (size_t)m, s));
            STEP_CK(hipMemsetAsync(B->bad, 0, sizeof(int) * (size_t)m, s));
            if ((rc = kernels(h, K, B, C.rec, unsupported)) || !unsupported.empty()) break;
            k_sp_out<<<blocks_for(m, 256), 256, 0, s>>>(m, B->rec, B->qb, B->cb, B->bad, K.valid, K.nonfinite, B->q, B->c, B->st);
            STEP_CK(hipGetLastError());
        }
        STEP_CK(hipMemcpyAsync(q, B->q, sizeof(long long) * (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(contacts, B->c, sizeof(long long) * (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(status, B->st, (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    if (refused) return fail(h, GRAAL_E_ARG, msg);
    return score_exit(h, K.fn, rc, unsupported.empty() ? nullptr : unsupported.c_str(), err);
}

} // namespace

extern "C" {

int graal_block_flips(graal_ctx* h, int32_t n_blocks, const int32_t* first, const int32_t* last, int64_t* q, int64_t* contacts, uint8_t* status)
{
    if (!h) return GRAAL_E_ARG;
    if (n_blocks < 0 || (n_blocks > 0 && (!first || !last || !q || !contacts || !status)))
        return fail(h, GRAAL_E_ARG, "graal_block_flips: n_blocks < 0 or a null array");
    return span_moves(h, SPAN_FLIPS, n_blocks, first, nullptr, last, q, contacts, status, sp_score);
}

int graal_block_swaps(graal_ctx* h, int32_t n_swaps, const int32_t* first, const int32_t* mid, const int32_t* last, int64_t* q, int64_t* contacts,
                      uint8_t* status)
{
    if (!h) return GRAAL_E_ARG;
    if (n_swaps < 0 || (n_swaps > 0 && (!first || !mid || !last || !q || !contacts || !status)))
        return fail(h, GRAAL_E_ARG, "graal_block_swaps: n_swaps < 0 or a null array");
    return span_moves(h, SPAN_SWAPS, n_swaps, first, mid, last, q, contacts, status, sp_score);
}

} // extern "C"
