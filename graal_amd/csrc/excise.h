// excise.h -- the likelihood cutting a run of fragments out of its contig would add, for a caller's set of disjoint spans in one pass
// (graal_block_excisions): the inverse of an insertion.  Included by graal_hip.hip after span_moves.h (it uses the records LnFrag /
// LnCtg, ln_block_add, ln_pair_mass, ln_quirk_pair, insert.h's in_shift_mass, span_moves.h's frame span_moves with SpanBuf and
// sp_unit_total, its sp_span_of, sp_add, sp_run_edges and sp_span_of_unit, span_check.h's SPAN_EXCISE and score_common.h's STEP_CK and
// stream_blocks).
//
// Span k = the fragments X of one linear contig at slots first .. last, bp interval [s0, e1), lx = e1 - s0; L = the contig's fragments
// before it, R = those behind it.  The excised layout leaves L as it is, gives every fragment of R start_bp - lx and pos - |X|, and makes X
// a linear contig of its own (direction and orientations kept, start_bp from 0); the float32 centres through centre_kb from the new
// integer starts.  E(k) = logL(excised) - logL(current) in the exact arithmetic with the roundings of junctions.h / links.h / insert.h:
//   X x (L u R)  every sub-fragment pair moves from its cis price to its trans price (v_inter * norm, the trans-branch RF-count indexing
//                under GRAAL_MODE_REF_TRANS_ACCU): a contact's term ob * (ln ex_trans - ln ex_cis) rounded to Q once; a fragment pair's
//                mass -(sum of ex_trans - ex_cis), X's fragment outer, rounded to Q once.  Beyond the window (gap > reach_bp) the cis
//                price is v_inter * plain norm: the difference is the indexing alone, the quirk term (junctions.h's, with a cut's sign);
//   L x R        every pair moves from its cis price at distance d to its cis price at d - lx, L's fragment outer.  A pair whose gap after
//                the excision -- the left fragment's distance to s0 plus the right one's to e1 -- is beyond reach_bp is v_inter * norm
//                both times: exactly 0, skipped.  A contact at >= d_max now and below it afterwards does contribute;
//   pairs inside X, inside L and inside R count as unchanged; nothing is reversed, so there is no mirror term.
// contacts[k] = the summed count of the X x (L u R) contacts whose current centre distance is below d_max: what the cut severs.
//
// The closing term's contacts.  A contact (a, b) of one contig changes price under EVERY scored span that lies strictly between its two
// slots and brings it inside the window; two routes were read for it:
//   (1) inside the streaming pass: a lane walks the sorted span list between the slots of its contact's two sides;
//   (2) insert.h's k_in_shift: a wave per span over the rows of the flank fragments within reach, through the row index.
// Route (1) is taken.  It needs no row index, so an unsorted contact list costs no device sort and no copy of the list (route 2 sorts it
// first, O(contacts) more memory); the list is read once for both terms where route 2 re-reads every row of a window once per span in
// reach of it -- with every fragment a span, a window's worth of reads per contact, most of them of partners that are not in R.  The
// walk is bounded by the call's longest span: a contact with d - max lx >= d_max (and 1 kb of slack for the float32 centres) feeds
// nothing and walks nothing; in a tiling of short spans the spans between a near-diagonal contact's sides are at most a window's worth,
// each of which it does feed.  Its cost shows only in a call that mixes one very long span with many short ones elsewhere in the
// same contig: contacts up to the long span's length apart walk the short spans between their sides and feed none.
//
// Kernels, all on the engine's stream:
//   span_moves' frame: k_jn_count / scan / k_ln_prep (recs_build) -- slots and per-slot records, as for links, insertions and span moves;
//   k_sp_gather -- per span of the caller its slots, labels, bp interval and contig; the host decides (span_check.h, kind 2): refuses the
//                 call, or sets aside the spans in a ring and those that are a whole contig and uploads the others sorted by first slot;
//   k_ex_sub    -- per fragment: the number of scored spans that start at or before its slot, its span and, per sub-fragment, a 32-byte
//                 record (two 16-byte loads) with its current centre;
//   k_ex_nnz    -- streams the contact list once, 64 consecutive contacts per wave.  X x rest: a contact of one contig whose sides differ
//                 in span feeds each side's span (cis -> trans, the count inside the window).  L x R: the lane walks the scored spans
//                 strictly between its two slots and prices the contact with the right side moved lx down.  Sums per run of equal span
//                 inside the wave (sp_add's run_sums) before the atomics; every loop bound around them is a wave ballot;
//   k_ex_edges / scan / k_ex_mass -- work units from a prefix sum, a wave per unit: (span, a fragment of X within reach of an end of X),
//                 which walks both flanks outwards from the boundaries 64 partners at a time, and (span, a fragment of L within reach of
//                 s0), which walks R outwards from e1 with what its own gap leaves of reach_bp; a walk stops when a whole step is out of
//                 reach.  A span with no R, or an L fragment beyond reach, has no unit of the second kind; one atomic per wave;
//   k_ex_quirk  -- only with the mode flag and mixed bins: a wave per span, lanes 8 x 8 (fragment of X, fragment of the contig outside X),
//                 the pairs beyond the window with a mixed bin (ln_quirk_pair, sign of a cut).  A span whose contig has no mixed bin
//                 returns at once;
//   k_sp_out    -- status and q per span, in the caller's order.
// No LDS.  hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage: VGPRs k_ex_sub 30, k_ex_nnz 78 (6 waves/SIMD),
// k_ex_edges 21, k_ex_mass 93 (5 waves/SIMD), k_ex_quirk 46; scratch 0 bytes/lane and no VGPR spill in each (k_ex_nnz and k_ex_mass
// keep 14 and 10 SGPRs in VGPR lanes).
#pragma once

namespace {

// ub: the scored spans whose first slot is <= this fragment's slot; span: the one that holds it, or -1
// acc: RF count | the bin's last RF count << 16; meta: sub k | fwd << 4
struct ExSub { float c_old; int label, slot, ub, span, frag, acc, meta; };
static_assert(sizeof(ExSub) == SPAN_SUB_BYTES, "a sub-fragment's record is two 16-byte loads");

__global__ __launch_bounds__(256) void k_ex_sub(int n, int m, const SpanRec* __restrict__ rec, const int* __restrict__ slot_of,
                                                const int* __restrict__ lab, const LnFrag* __restrict__ fr, const int* __restrict__ sub_ids,
                                                ExSub* __restrict__ sub)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int slot = slot_of[f];
    if (slot < 0 || slot >= n) return;                               // (a corrupt layout: refused before anything reads the records)
    const LnFrag x = fr[slot];
    int lo = 0;
    const int j = sp_span_of(rec, m, slot, &lo);
    const bool fo = x.fwd != 0;
    const int last = stat_accu(x.st, x.st.n - 1);
    int4 ids = make_int4(f, 0, 0, 1);
    if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[f];
    for (int k = 0; k < x.st.n; k++) {
        ExSub u;
        u.c_old = centre_kb(x.start, fo, x.st, k);
        u.label = lab[f]; u.slot = slot; u.ub = lo; u.span = j; u.frag = f;
        u.acc = stat_accu(x.st, k) | (last << 16);                   // (RF counts are <= 30000)
        u.meta = k | ((fo ? 1 : 0) << 4);
        sub[sel3(ids.x, ids.y, ids.z, k)] = u;
    }
}

// far_kb: the call's longest span in kb plus 1 kb of slack: a contact with d - far_kb >= d_max closes under no span of the call
__global__ __launch_bounds__(256) void k_ex_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt, long long nnz,
                                                const ExSub* __restrict__ sub, const SpanRec* __restrict__ rec, const LnFrag* __restrict__ fr,
                                                float nfpb, Par par, int quirk, float far_kb, long long* __restrict__ qb,
                                                long long* __restrict__ cb, int* __restrict__ badb)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {   // (wave-uniform bounds: the run sums need the whole wave)
        const long long k = k0 + lane;
        unsigned long long ka = LN_EMPTY, kb = LN_EMPTY;
        long long qx = 0, cx = 0, bx = 0;                            // the X x rest term: the same for the span of either side
        int ja = 0, jend = 0, k_hi = 0;                              // the scored spans strictly between the two sides
        float c_lo = 0.0f, ex_old = 0.0f, norm = 0.0f;
        double ob = 0.0;
        LnFrag Y = {};
        if (k < nnz) {
            const ExSub A = sub[row[k]], B = sub[col[k]];
            if (A.label == B.label && A.slot != B.slot) {
                ob = (double)__int_as_float(cnt[k]);
                const int own_a = A.acc & 0xffff, own_b = B.acc & 0xffff;
                norm = (float)(own_a * own_b) / nfpb;
                const float sd = fabsf(B.c_old - A.c_old);
                ex_old = rippe(sd, par) * norm;
                if (A.span != B.span) {
                    int prod_t = own_a * own_b;                      // the trans indexing: the lower-id bin's orientation picks its RF count
                    if (quirk) prod_t = A.frag < B.frag ? (((A.meta >> 4) & 1) ? own_a : (A.acc >> 16)) * own_b
                                                        : own_a * (((B.meta >> 4) & 1) ? own_b : (B.acc >> 16));
                    const float ex_t = par.v_inter * ((float)prod_t / nfpb);
                    if (sd < par.d_max) cx = (long long)llrint(ob);
                    if (ex_t != ex_old) {
                        const long long t = to_q(ob * (mm_ln(ex_t) - mm_ln(ex_old)));
                        if (t == Q_BAD) bx = 1; else qx = t;
                    }
                    if (A.span >= 0) ka = (unsigned long long)A.span;
                    if (B.span >= 0) kb = (unsigned long long)B.span;
                }
                const bool a_low = A.slot < B.slot;
                const ExSub& lo = a_low ? A : B;
                const ExSub& hi = a_low ? B : A;
                if (!(sd - far_kb >= par.d_max)) {
                    ja = lo.ub; jend = hi.ub - (hi.span >= 0 ? 1 : 0);
                    if (ja < jend) { Y = fr[hi.slot]; c_lo = lo.c_old; k_hi = hi.meta & 3; }
                }
            }
        }
        if (__ballot(ka != LN_EMPTY) != 0ull) sp_add(ka, qx, cx, bx, qb, cb, badb);
        if (__ballot(kb != LN_EMPTY) != 0ull) sp_add(kb, qx, cx, bx, qb, cb, badb);
        for (int t = 0; ; t++) {
            const int j = ja + t;
            const bool live = j < jend;
            if (__ballot(live) == 0ull) break;
            unsigned long long key = LN_EMPTY;
            long long q = 0, c = 0, bad = 0;
            if (live) {
                const SpanRec b = rec[j];
                const float c_new = centre_kb(Y.start - (b.e1 - b.s0), Y.fwd != 0, Y.st, k_hi);
                const float ex_new = rippe(fabsf(c_new - c_lo), par) * norm;
                if (ex_new != ex_old) {                              // (else both beyond the window)
                    const long long v = to_q(ob * (mm_ln(ex_new) - mm_ln(ex_old)));
                    if (v == Q_BAD) bad = 1; else q = v;
                    key = (unsigned long long)j;
                }
            }
            if (__ballot(key != LN_EMPTY) != 0ull) sp_add(key, q, c, bad, qb, cb, badb);
        }
    }
}

// per span: ne = its work units, nx = (units of X, of them counted from the left, fragments of L within reach of s0 when there is an R)
__global__ void k_ex_edges(int m, const SpanRec* __restrict__ rec, const LnFrag* __restrict__ fr, int reach_bp, long long* __restrict__ ne,
                           int4* __restrict__ nx)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > m) return;
    if (j == m) { ne[m] = 0; return; }                               // (the scan's last entry: the total)
    const SpanRec b = rec[j];
    const int2 x = sp_run_edges(fr, b.first, b.last, b.s0, b.e1, reach_bp);
    int lo = 0;
    if (b.last < b.clast) {
        int hi = b.first - b.cfirst;                                 // first u (counted from slot first - 1 down) with gap > reach
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const LnFrag y = fr[b.first - 1 - mid];
            if ((long long)b.s0 - ((long long)y.start + y.len) <= reach_bp) lo = mid + 1; else hi = mid;
        }
    }
    ne[j] = (long long)x.x + lo;
    nx[j] = make_int4(x.x, x.y, lo, 0);
}

// One walk of a unit's fragment x: partners from slot `from` in steps of `dir` while inside [lo_slot, hi_slot] and their gap to the
// boundary `edge` they are walked away from is <= budget (the gap only grows).  lx 0: x in X, the pair goes from cis to trans; lx > 0: x
// in L, the partner in R moves lx bp down, cis both times.
__device__ __forceinline__ void ex_walk(const LnFrag* __restrict__ fr, int from, int dir, int lo_slot, int hi_slot, int edge, long long budget, int lx,
                                        const LnFrag& x, float nfpb, const Par& par, int quirk, long long& sum, long long& nb)
{
    if (budget < 0) return;                                          // (wave-uniform)
    const int lane = threadIdx.x & 63;
    for (long long t = lane; ; t += 64) {
        const long long i = (long long)from + dir * t;
        bool in = i >= lo_slot && i <= hi_slot;
        LnFrag y;
        if (in) {
            y = fr[i];
            const long long g = dir < 0 ? (long long)edge - ((long long)y.start + y.len) : (long long)y.start - edge;
            in = g <= budget;
        }
        if (__ballot(in) == 0ull) break;
        if (in) {
            // E's mass is -(sum of ex_new - ex_old): ln_pair_mass sums ex_cis - ex_trans = old - new, in_shift_mass new - old
            const long long q = lx ? to_q_fast(in_shift_mass(x, y, -lx, nfpb, par))
                                   : to_q_fast(ln_pair_mass(x, x.start, x.fwd != 0, y, y.start, y.fwd != 0, nfpb, par, quirk));
            if (q == Q_BAD) nb++; else sum += lx ? -q : q;
        }
    }
}

__global__ __launch_bounds__(256) void k_ex_mass(long long total, int m, const SpanRec* __restrict__ rec, const long long* __restrict__ noff,
                                                 const long long* __restrict__ ne, const int4* __restrict__ nx, const LnFrag* __restrict__ fr,
                                                 float nfpb, Par par, int quirk, int reach_bp, long long* __restrict__ qb, int* __restrict__ badb)
{
    const long long W = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (W >= total) return;                                          // (wave-uniform)
    const int j = sp_span_of_unit(noff, m, W);
    const long long u = W - noff[j];
    if (u < 0 || u >= ne[j]) return;
    const SpanRec b = rec[j];
    const int4 e = nx[j];
    long long sum = 0, nb = 0;
    if (u < e.x) {                                                   // a fragment of X against both flanks
        const int slot = u < e.y ? b.first + (int)u : b.last - (int)(u - e.y);
        if (slot < b.first || slot > b.last) return;
        const LnFrag x = fr[slot];
        const long long l0 = (long long)x.start - b.s0, r0 = (long long)b.e1 - ((long long)x.start + x.len);
        ex_walk(fr, b.first - 1, -1, b.cfirst, b.first - 1, b.s0, reach_bp - l0, 0, x, nfpb, par, quirk, sum, nb);
        ex_walk(fr, b.last + 1, 1, b.last + 1, b.clast, b.e1, reach_bp - r0, 0, x, nfpb, par, quirk, sum, nb);
    } else {                                                         // a fragment of L against R: its gap after the excision is gl + gr
        const int slot = b.first - 1 - (int)(u - e.x);
        if (slot < b.cfirst || slot >= b.first || b.e1 <= b.s0) return;
        const LnFrag x = fr[slot];
        const long long gl = (long long)b.s0 - ((long long)x.start + x.len);
        ex_walk(fr, b.last + 1, 1, b.last + 1, b.clast, b.e1, reach_bp - gl, b.e1 - b.s0, x, nfpb, par, 0, sum, nb);
    }
    ln_block_add(sum, nb, &qb[j], &badb[j]);
}

// GRAAL_MODE_REF_TRANS_ACCU with mixed bins: a wave per span over X x the rest of its contig.  A pair beyond the window with a mixed bin
// is v_inter * plain norm now and v_inter * indexed norm once the cut separates it: ln_quirk_pair's term for a join, with the other sign.
__global__ __launch_bounds__(256) void k_ex_quirk(int m, const SpanRec* __restrict__ rec, const LnFrag* __restrict__ fr, const int* __restrict__ lab,
                                                  const LnCtg* __restrict__ ctg, float nfpb, Par par, int reach_bp, long long* __restrict__ qb,
                                                  int* __restrict__ badb)
{
    const int lane = threadIdx.x & 63;
    const int W = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (W >= m) return;                                              // (wave-uniform)
    const SpanRec b = rec[W];
    if (ctg[lab[fr[b.first].frag]].nmix == 0) return;
    const int jl = lane & 7, nx = b.last - b.first + 1, rest = (b.clast - b.cfirst + 1) - nx;
    long long sum = 0, nb = 0;
    for (int g = 0; g * 8 < nx; g++) {
        const int i = g * 8 + (lane >> 3);
        if (i >= nx) continue;
        const LnFrag x = fr[b.first + i];
        const bool mx = !stat_uniform(x.st);
        for (int r = jl; r < rest; r += 8) {
            const int ys = b.cfirst + r < b.first ? b.cfirst + r : r + nx + b.cfirst;   // (the contig's slots with X left out)
            const LnFrag y = fr[ys];
            if (!mx && stat_uniform(y.st)) continue;
            const long long gap = ys < b.first ? (long long)x.start - ((long long)y.start + y.len) : (long long)y.start - ((long long)x.start + x.len);
            if (gap <= reach_bp) continue;
            long long s = 0;
            ln_quirk_pair(x, y, true, false, false, nfpb, par, s, nb);
            sum -= s;
        }
    }
    ln_block_add(sum, nb, &qb[W], &badb[W]);
}

// The kernels of an excision: what span_moves runs between the upload of the scored spans `rec` and k_sp_out.
int ex_score(graal_ctx* h, const SpanKind& K, SpanBuf* B, const std::vector<SpanRec>& rec, std::string& unsupported)
{
    const int n = h->n, m = (int)rec.size();
    const LayoutRecs& R = B->R;
    ExSub* const sub = (ExSub*)B->sub.p;
    hipStream_t s = h->stream;
    const int quirk = (h->mode & GRAAL_MODE_REF_TRANS_ACCU) ? 1 : 0;
    const int reach = reach_bp(h);
    long long max_lx = 0;
    for (const SpanRec& r : rec) max_lx = std::max(max_lx, (long long)r.e1 - r.s0);
    const float far_kb = (float)((double)max_lx / 1000.0 + 1.0);
    int rc = GRAAL_OK;
    do {
        k_ex_sub<<<blocks_for(n, 256), 256, 0, s>>>(n, m, B->rec, R.L.slot, R.lab, R.fr, h->d_sub_ids, sub);
        STEP_CK(hipGetLastError());
        if (h->nnz > 0) {
            k_ex_nnz<<<stream_blocks(h->nnz), 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, sub, B->rec, R.fr, h->nfpb, h->par, quirk, far_kb, B->qb,
                                                           B->cb, B->bad);
            STEP_CK(hipGetLastError());
        }
        k_ex_edges<<<blocks_for(m + 1, 256), 256, 0, s>>>(m, B->rec, R.fr, reach, B->ne, B->nx);
        STEP_CK(hipGetLastError());
        long long total = 0;                                          // (<= fragments of the spans + spans x a window's fragments)
        if ((rc = sp_unit_total(h, B, m, total))) break;
        if ((total + 3) / 4 > (long long)INT_MAX) {
            char msg[240];
            snprintf(msg, sizeof msg, "%s: %lld work units exceed one launch: score fewer spans per call", K.fn, total);
            unsupported = msg;
            break;
        }
        if (total > 0) {
            k_ex_mass<<<(unsigned)((total + 3) / 4), 256, 0, s>>>(total, m, B->rec, B->noff, B->ne, B->nx, R.fr, h->nfpb, h->par, quirk, reach,
                                                                 B->qb, B->bad);
            STEP_CK(hipGetLastError());
        }
        if (quirk && h->n_ubins) {
            k_ex_quirk<<<blocks_for(m, 4), 256, 0, s>>>(m, B->rec, R.fr, R.lab, R.ctg, h->nfpb, h->par, reach, B->qb, B->bad);
            STEP_CK(hipGetLastError());
        }
    } while (false);
    return rc;
}

} // namespace

extern "C" {

int graal_block_excisions(graal_ctx* h, int32_t n_spans, const int32_t* first, const int32_t* last, int64_t* q, int64_t* contacts, uint8_t* status)
{
    if (!h) return GRAAL_E_ARG;
    if (n_spans < 0 || (n_spans > 0 && (!first || !last || !q || !contacts || !status)))
        return fail(h, GRAAL_E_ARG, "graal_block_excisions: n_spans < 0 or a null array");
    return span_moves(h, SPAN_EXCISE, n_spans, first, nullptr, last, q, contacts, status, ex_score);
}

} // extern "C"
