// swaps.h -- the likelihood each swap of two adjacent runs of a contig would add, for a caller's set of disjoint spans in one pass
// (graal_block_swaps).  Included by graal_hip.hip after flips.h (it uses LayoutRecs with recs_reserve / recs_build, the records LnFrag /
// LnCtg, ln_run_sum, ln_block_add, fl_contact, fl_add and score_common.h's score_entry, score_exit, STEP_CK and free_null).
//
// Swap k = two adjacent runs of one contig: X at positions pos[first[k]] .. pos[mid[k]] and Y at pos[mid[k]] + 1 .. pos[last[k]], in the
// bp interval [s0, e1) with the breakpoint sm between them (lx = sm - s0, ly = e1 - sm).  The swapped layout puts Y first: a fragment of
// X moves ly bp up, a fragment of Y lx bp down, ori and every other field stay; the float32 centres through centre_kb from the new integer
// starts.  S(k) = logL(swapped) - logL(current) in the exact arithmetic with the roundings of junctions.h / links.h / flips.h: pairs
// inside X, inside Y and outside X u Y count as unchanged; every sub-fragment pair of X x Y, X x rest and Y x rest (rest: the contig's
// other fragments) moves from its cis price to its cis price in the swapped layout
//   a contact:                ob * (ln ex_new - ln ex_old), rounded to Q once per contact (0 where the two prices are the same float32);
//   a fragment pair's mass:   -(sum over its sub-fragment pairs of ex_new - ex_old), the moved run's fragment outer (X's for X x Y),
//                             rounded to Q once.
// A fragment x of a run lies dl bp behind its run's left end and dr bp before its right end.  With g the gap of a flank fragment to the
// span's boundary it faces, the pair's gap is, before and after the swap,
//   x in X, left flank:  dl + g        and dl + ly + g        x in X, right flank: dr + ly + g  and dr + g
//   x in Y, left flank:  dl + lx + g   and dl + g             x in Y, right flank: dr + g       and dr + lx + g
//   x in X, y in Y:      dr(x) + dl(y) and dl(x) + dr(y)
// so a pair is beyond the window both times -- priced v_inter * norm twice, difference exactly 0 -- unless the smaller of the two is
// <= reach_bp: only the run fragments within reach of one of their run's ends, and partners within reach of a breakpoint, take part, at
// most about (4w) x (3w) fragment pairs per swap however long the runs.  Orientation does not change and cis prices do not use the
// trans-branch indexing: GRAAL_MODE_REF_TRANS_ACCU changes nothing, there is no mirror pass.
//
// Every fragment belongs to at most one span, so a contact feeds at most two sums and the list is streamed once; no candidate table.
// Kernels, all on the engine's stream:
//   k_jn_count / scan / k_ln_prep (recs_build) -- slots and per-slot records, as for links, insertions and flips;
//   k_sw_gather -- per swap of the caller: the slots and labels of its three fragments, its bp interval and breakpoint, its contig's slots.
//                 The host validates from these (two contigs, wrong order, overlap: an ordered set of the spans so far), sets aside the
//                 swaps in a ring, and uploads the others sorted by first slot;
//   k_sw_sub    -- per fragment: its swap (binary search over the sorted spans), its role (X or Y) and, per sub-fragment, a 32-byte record
//                 with its current and its swapped centre;
//   k_sw_nnz    -- streams the contact list once, 64 consecutive contacts per wave.  A contact of one contig is priced once for its swap
//                 when its sides are X and Y of the same swap (both moved), and once per side whose swap differs from the other side's,
//                 with that side moved alone.  Sums per run of equal swap inside the wave (ln_run_sum) before the atomics;
//   k_sw_edges / scan / k_sw_mass -- work units (swap, one fragment of X or Y within reach of an end of its run) from a prefix sum, a wave
//                 per unit; its lanes walk the partner ranges outwards from the breakpoints 64 fragments at a time and stop when a whole
//                 step is out of reach in both layouts; one atomic per wave;
//   k_sw_out    -- status and q per swap, in the caller's order.
#pragma once

namespace {

struct SwSub { float c_old, c_new; int label, sw, role, acc, pad0, pad1; };   // role: 0 in X, 1 in Y; acc: the sub-fragment's RF count
struct SwInfo { int slot_f, slot_m, slot_l, lab_f, lab_m, lab_l, s0, sm, e1, cfirst, ccnt, circ; };   // per swap of the caller
struct SwRec { int s0, sm, e1, first, mid, last, cfirst, clast, id, pad; };   // the scored swaps, sorted by first slot; id: the caller's index

struct SwBuf {
    LayoutRecs R;
    SwSub* sub = nullptr; int n = 0, S = 0;                           // per sub-fragment
    int *first = nullptr, *mid = nullptr, *last = nullptr; SwInfo* info = nullptr; SwRec* rec = nullptr;
    long long *qb = nullptr, *cb = nullptr, *q = nullptr, *c = nullptr; int *bad = nullptr, *ne = nullptr, *noff = nullptr; int4* nx = nullptr;
    unsigned char* st = nullptr;
    void* tmp = nullptr; size_t tmp_bytes = 0;
    size_t bcap = 0;                                                  // swaps the per-swap arrays hold
};

void sw_free_swaps(SwBuf* b)
{
    free_null({(void**)&b->first, (void**)&b->mid, (void**)&b->last, (void**)&b->info, (void**)&b->rec, (void**)&b->qb, (void**)&b->cb,
               (void**)&b->q, (void**)&b->c, (void**)&b->bad, (void**)&b->ne, (void**)&b->noff, (void**)&b->nx, (void**)&b->st, &b->tmp});
    b->bcap = 0; b->tmp_bytes = 0;
}

void sw_free_subs(SwBuf* b)
{
    free_null({(void**)&b->sub});
    b->n = 0; b->S = 0;
}

void sw_free(SwBuf* b)
{
    if (!b) return;
    recs_free(b->R); sw_free_subs(b); sw_free_swaps(b);
    delete b;
}

__global__ void k_sw_gather(int nb, int n, const int* __restrict__ first, const int* __restrict__ mid, const int* __restrict__ last,
                            const int* __restrict__ slot_of, const int* __restrict__ lab, const LnFrag* __restrict__ fr,
                            const LnCtg* __restrict__ ctg, SwInfo* __restrict__ info)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    SwInfo r = {-1, -1, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0};
    const int f = first[k], m = mid[k], l = last[k];                 // (in [0, n): the host checked)
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

// the scored swap whose span holds `slot`, or -1: the last span that starts at or before it, if it reaches that far
__device__ __forceinline__ int sw_swap_of(const SwRec* __restrict__ rec, int m, int slot)
{
    int lo = 0, hi = m;                                              // first span with .first > slot
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rec[mid].first <= slot) lo = mid + 1; else hi = mid;
    }
    return (lo > 0 && slot <= rec[lo - 1].last) ? lo - 1 : -1;
}

__global__ __launch_bounds__(256) void k_sw_sub(int n, int m, const SwRec* __restrict__ rec, const int* __restrict__ slot_of, const int* __restrict__ lab,
                                                const LnFrag* __restrict__ fr, const int* __restrict__ sub_ids, SwSub* __restrict__ sub)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int slot = slot_of[f];
    if (slot < 0 || slot >= n) return;                               // (a corrupt layout: refused before anything reads the records)
    const LnFrag x = fr[slot];
    const int j = sw_swap_of(rec, m, slot);
    int ns = x.start, role = 0;
    if (j >= 0) {
        const SwRec b = rec[j];
        role = slot > b.mid ? 1 : 0;
        ns = role ? x.start - (b.sm - b.s0) : x.start + (b.e1 - b.sm);   // (inside [s0, e1): no overflow)
    }
    int4 ids = make_int4(f, 0, 0, 1);
    if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[f];
    for (int k = 0; k < x.st.n; k++) {
        SwSub u;
        u.c_old = centre_kb(x.start, x.fwd != 0, x.st, k);
        u.c_new = j >= 0 ? centre_kb(ns, x.fwd != 0, x.st, k) : u.c_old;
        u.label = lab[f]; u.sw = j; u.role = role; u.acc = stat_accu(x.st, k); u.pad0 = 0; u.pad1 = 0;
        sub[sel3(ids.x, ids.y, ids.z, k)] = u;
    }
}

__global__ __launch_bounds__(256) void k_sw_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt, long long nnz,
                                                const SwSub* __restrict__ sub, float nfpb, Par par, long long* __restrict__ qb,
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
            const SwSub A = sub[row[k]], B = sub[col[k]];
            if (A.label == B.label && (A.sw != B.sw || (A.sw >= 0 && A.role != B.role))) {   // (sub-fragments of one bin share swap and role)
                const double ob = (double)__int_as_float(cnt[k]);
                const float norm = (float)(A.acc * B.acc) / nfpb;
                const float ex_old = rippe(fabsf(B.c_old - A.c_old), par) * norm;
                if (A.sw == B.sw) { ka = (unsigned long long)A.sw; fl_contact(fabsf(B.c_new - A.c_new), ex_old, norm, ob, par, qa, ca, ba); }
                else {
                    if (A.sw >= 0) { ka = (unsigned long long)A.sw; fl_contact(fabsf(B.c_old - A.c_new), ex_old, norm, ob, par, qa, ca, ba); }
                    if (B.sw >= 0) { kb = (unsigned long long)B.sw; fl_contact(fabsf(B.c_new - A.c_old), ex_old, norm, ob, par, qc, cc, bc); }
                }
            }
        }
        if (__ballot(ka != LN_EMPTY) != 0ull) fl_add(ka, qa, ca, ba, qb, cb, badb);
        if (__ballot(kb != LN_EMPTY) != 0ull) fl_add(kb, qc, cc, bc, qb, cb, badb);
    }
}

// the fragments of the run of slots [a, b] in the bp interval [lo_bp, hi_bp) within reach of an end: (units, those counted from the left);
// all of them when the two groups meet.  Starts grow with the slot, so both counts come from binary searches.
__device__ __forceinline__ int2 sw_run_edges(const LnFrag* __restrict__ fr, int a, int b, int lo_bp, int hi_bp, int reach_bp)
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

// per swap: the units of X and of Y (nx = units of X, of them from the left, units of Y, of them from the left); ne = their sum
__global__ void k_sw_edges(int m, const SwRec* __restrict__ rec, const LnFrag* __restrict__ fr, int reach_bp, int* __restrict__ ne, int4* __restrict__ nx)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > m) return;
    if (j == m) { ne[m] = 0; return; }                               // (the scan's last entry: the total)
    const SwRec b = rec[j];
    const int2 x = sw_run_edges(fr, b.first, b.mid, b.s0, b.sm, reach_bp), y = sw_run_edges(fr, b.mid + 1, b.last, b.sm, b.e1, reach_bp);
    ne[j] = x.x + y.x;
    nx[j] = make_int4(x.x, x.y, y.x, y.y);
}

// mass term of the moved fragment x (current centres xo, swapped centres xn) and a partner y that sits at y.start now and at ys_new in the
// swapped layout: -(sum of ex_new - ex_old), x outer
__device__ __forceinline__ long long sw_pair_q(const LnFrag& x, float xo0, float xo1, float xo2, float xn0, float xn1, float xn2, const LnFrag& y,
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

// the unit's swap: the last j with noff[j] <= W (every swap has at least two units)
__device__ __forceinline__ int sw_swap_of_unit(const int* __restrict__ noff, int m, int W)
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
// skip_budget was priced by an earlier walk (X x Y only; skip_budget < 0: none).  shift: what the swap adds to the partner's start.
__device__ __forceinline__ void sw_walk(const LnFrag* __restrict__ fr, int from, int dir, int lo_slot, int hi_slot, int edge, long long budget,
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
            const long long q = sw_pair_q(x, xo0, xo1, xo2, xn0, xn1, xn2, y, y.start + shift, nfpb, par);
            if (q == Q_BAD) nb++; else sum -= q;
        }
    }
}

__global__ __launch_bounds__(256) void k_sw_mass(int total, int m, const SwRec* __restrict__ rec, const int* __restrict__ noff, const int* __restrict__ ne,
                                                 const int4* __restrict__ nx, const LnFrag* __restrict__ fr, float nfpb, Par par, int reach_bp,
                                                 long long* __restrict__ qb, int* __restrict__ badb)
{
    const int W = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (W >= total) return;                                          // (wave-uniform)
    const int j = sw_swap_of_unit(noff, m, W);
    int u = W - noff[j];
    if (u < 0 || u >= ne[j]) return;
    const SwRec b = rec[j];
    const int4 e = nx[j];
    const bool in_y = u >= e.x;
    if (in_y) u -= e.x;
    const int left = in_y ? e.w : e.y;
    const int ra = in_y ? b.mid + 1 : b.first, rb = in_y ? b.last : b.mid;   // the unit's run
    const int slot = u < left ? ra + u : rb - (u - left);
    if (slot < ra || slot > rb) return;
    const LnFrag x = fr[slot];
    const int lx = b.sm - b.s0, ly = b.e1 - b.sm;
    const long long dl = (long long)x.start - (in_y ? b.sm : b.s0), dr = (long long)(in_y ? b.e1 : b.sm) - ((long long)x.start + x.len);
    const int ns = in_y ? x.start - lx : x.start + ly;
    const bool fo = x.fwd != 0;
    const float xo0 = centre_kb(x.start, fo, x.st, 0), xo1 = x.st.n > 1 ? centre_kb(x.start, fo, x.st, 1) : 0.0f,
                xo2 = x.st.n > 2 ? centre_kb(x.start, fo, x.st, 2) : 0.0f;
    const float xn0 = centre_kb(ns, fo, x.st, 0), xn1 = x.st.n > 1 ? centre_kb(ns, fo, x.st, 1) : 0.0f,
                xn2 = x.st.n > 2 ? centre_kb(ns, fo, x.st, 2) : 0.0f;
    long long sum = 0, nb = 0;
    // the flanks: the smaller of a pair's two gaps is dl + g on the left for X (now) and for Y (swapped), dr + g on the right
    sw_walk(fr, b.first - 1, -1, b.cfirst, b.first - 1, b.s0, reach_bp - dl, 0, -1, 0, x, xo0, xo1, xo2, xn0, xn1, xn2, nfpb, par, sum, nb);
    sw_walk(fr, b.last + 1, 1, b.last + 1, b.clast, b.e1, reach_bp - dr, 0, -1, 0, x, xo0, xo1, xo2, xn0, xn1, xn2, nfpb, par, sum, nb);
    if (!in_y) {
        // X x Y: now the gap is dr(x) + dl(y), walked from Y's left end; swapped it is dl(x) + dr(y), walked from Y's right end, less
        // the pairs the first walk took
        sw_walk(fr, b.mid + 1, 1, b.mid + 1, b.last, b.sm, reach_bp - dr, 0, -1, -lx, x, xo0, xo1, xo2, xn0, xn1, xn2, nfpb, par, sum, nb);
        sw_walk(fr, b.last, -1, b.mid + 1, b.last, b.e1, reach_bp - dl, b.sm, reach_bp - dr, -lx, x, xo0, xo1, xo2, xn0, xn1, xn2, nfpb, par,
                sum, nb);
    }
    ln_block_add(sum, nb, &qb[j], &badb[j]);
}

__global__ void k_sw_out(int m, const SwRec* __restrict__ rec, const long long* __restrict__ qb, const long long* __restrict__ cb,
                         const int* __restrict__ badb, long long* __restrict__ q, long long* __restrict__ c, unsigned char* __restrict__ st)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int id = rec[j].id;
    const bool bad = badb[j] != 0;
    st[id] = bad ? GRAAL_SWAP_NONFINITE : GRAAL_SWAP_VALID;
    q[id] = bad ? 0 : qb[j];
    c[id] = cb[j];
}

} // namespace

extern "C" {

int graal_block_swaps(graal_ctx* h, int32_t n_swaps, const int32_t* first, const int32_t* mid, const int32_t* last, int64_t* q, int64_t* contacts,
                      uint8_t* status)
{
    if (!h) return GRAAL_E_ARG;
    if (n_swaps < 0 || (n_swaps > 0 && (!first || !mid || !last || !q || !contacts || !status)))
        return fail(h, GRAAL_E_ARG, "graal_block_swaps: n_swaps < 0 or a null array");
    if (const int rc = score_entry(h, "graal_block_swaps")) return rc;
    if (n_swaps == 0) return GRAAL_OK;
    const int n = h->n, S = h->n_sub_total, nb = n_swaps;
    char msg[240];
    for (int k = 0; k < nb; k++)
        if (first[k] < 0 || first[k] >= n || mid[k] < 0 || mid[k] >= n || last[k] < 0 || last[k] >= n) {
            snprintf(msg, sizeof msg, "graal_block_swaps: swap %d: fragment index out of range (%d, %d, %d; %d fragments)", k, first[k], mid[k],
                     last[k], n);
            return fail(h, GRAAL_E_ARG, msg);
        }
    if (!h->sw) h->sw = new SwBuf();
    SwBuf* B = h->sw;
    LayoutRecs& R = B->R;
    hipStream_t s = h->stream;
    if (const int rc = recs_reserve(h, R)) return rc;
    if (B->n != n || B->S != S) {                                     // (B->n stays 0 until the set is allocated)
        sw_free_subs(B);
        CK(hipMalloc(&B->sub, sizeof(SwSub) * (size_t)std::max(S, 1)));
        B->n = n; B->S = S;
    }
    if ((size_t)nb > B->bcap) {                                       // (grows to the largest call; bcap stays 0 until the set is allocated)
        sw_free_swaps(B);
        const size_t cap = (size_t)nb + 1;
        CK(hipMalloc(&B->first, sizeof(int) * cap));
        CK(hipMalloc(&B->mid, sizeof(int) * cap));
        CK(hipMalloc(&B->last, sizeof(int) * cap));
        CK(hipMalloc(&B->info, sizeof(SwInfo) * cap));
        CK(hipMalloc(&B->rec, sizeof(SwRec) * cap));
        CK(hipMalloc(&B->qb, sizeof(long long) * cap));
        CK(hipMalloc(&B->cb, sizeof(long long) * cap));
        CK(hipMalloc(&B->q, sizeof(long long) * cap));
        CK(hipMalloc(&B->c, sizeof(long long) * cap));
        CK(hipMalloc(&B->bad, sizeof(int) * cap));
        CK(hipMalloc(&B->ne, sizeof(int) * cap));
        CK(hipMalloc(&B->noff, sizeof(int) * cap));
        CK(hipMalloc(&B->nx, sizeof(int4) * cap));
        CK(hipMalloc(&B->st, cap));
        size_t tb = 0;
        CK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, B->ne, B->noff, (int)cap, s));
        CK(hipMalloc(&B->tmp, tb));
        B->tmp_bytes = tb;
        B->bcap = (size_t)nb;
    }
    int rc = GRAAL_OK;
    unsigned err = 0;
    bool refused = false;
    std::vector<SwInfo> info((size_t)nb);
    std::vector<SwRec> rec;
    std::vector<unsigned char> st((size_t)nb);
    do {
        if ((rc = recs_build(h, R, 1))) break;
        STEP_CK(hipMemcpyAsync(B->first, first, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, s));
        STEP_CK(hipMemcpyAsync(B->mid, mid, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, s));
        STEP_CK(hipMemcpyAsync(B->last, last, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, s));
        k_sw_gather<<<blocks_for(nb, 256), 256, 0, s>>>(nb, n, B->first, B->mid, B->last, R.slot, R.lab, R.fr, R.ctg, B->info);
        STEP_CK(hipGetLastError());
        STEP_CK(hipMemcpyAsync(&err, R.err, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(info.data(), B->info, sizeof(SwInfo) * (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
        if (err) break;   // (a corrupt layout: the slots are not to be trusted, nothing reads them)
        // ---- validation: the first offending swap, by the caller's numbering
        int off = nb;
        const char* what = nullptr;
        // (overlap: the spans enter an ordered set in the caller's order; those already in it are pairwise disjoint, so the first span
        // that meets one of its two neighbours there is the first that overlaps an earlier span)
        std::map<int, int> by_first;                                  // first slot -> last slot
        for (int k = 0; k < nb && off == nb; k++) {
            const SwInfo& I = info[(size_t)k];
            if (I.slot_f < 0) { off = k; what = "a fragment without a slot"; }
            else if (I.lab_f != I.lab_m || I.lab_f != I.lab_l) { off = k; what = "first, mid and last lie on two contigs"; }
            else if (I.slot_f > I.slot_m) { off = k; what = "mid lies before first"; }
            else if (I.slot_m >= I.slot_l) { off = k; what = "last does not lie behind mid"; }
            else {
                auto nx = by_first.lower_bound(I.slot_f);             // the first span that starts at or behind this one
                bool hit = nx != by_first.end() && nx->first <= I.slot_l;
                if (!hit && nx != by_first.begin()) hit = std::prev(nx)->second >= I.slot_f;
                if (hit) { off = k; what = "overlaps an earlier swap"; }
                else by_first.emplace(I.slot_f, I.slot_l);
            }
        }
        if (off != nb) {
            snprintf(msg, sizeof msg, "graal_block_swaps: swap %d (fragments %d .. %d .. %d): %s", off, first[off], mid[off], last[off], what);
            refused = true;
            break;
        }
        std::vector<int> order((size_t)nb);
        for (int k = 0; k < nb; k++) order[(size_t)k] = k;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return info[(size_t)a].slot_f < info[(size_t)b].slot_f; });
        // ---- the scored swaps, sorted by first slot; those in a ring have their status already
        for (int i = 0; i < nb; i++) {
            const int k = order[(size_t)i];
            const SwInfo& I = info[(size_t)k];
            if (I.circ) { st[(size_t)k] = GRAAL_SWAP_CIRCULAR; continue; }
            st[(size_t)k] = GRAAL_SWAP_VALID;
            rec.push_back(SwRec{I.s0, I.sm, I.e1, I.slot_f, I.slot_m, I.slot_l, I.cfirst, I.cfirst + I.ccnt - 1, k, 0});
        }
        const int m = (int)rec.size();
        STEP_CK(hipMemsetAsync(B->q, 0, sizeof(long long) * (size_t)nb, s));
        STEP_CK(hipMemsetAsync(B->c, 0, sizeof(long long) * (size_t)nb, s));
        STEP_CK(hipMemcpyAsync(B->st, st.data(), (size_t)nb, hipMemcpyHostToDevice, s));
        if (m > 0) {
            STEP_CK(hipMemcpyAsync(B->rec, rec.data(), sizeof(SwRec) * (size_t)m, hipMemcpyHostToDevice, s));
            STEP_CK(hipMemsetAsync(B->qb, 0, sizeof(long long) * (size_t)m, s));
            STEP_CK(hipMemsetAsync(B->cb, 0, sizeof(long long) * (size_t)m, s));
            STEP_CK(hipMemsetAsync(B->bad, 0, sizeof(int) * (size_t)m, s));
            k_sw_sub<<<blocks_for(n, 256), 256, 0, s>>>(n, m, B->rec, R.slot, R.lab, R.fr, h->d_sub_ids, B->sub);
            STEP_CK(hipGetLastError());
            if (h->nnz > 0) {
                const long long waves = (h->nnz + 63) / 64;
                const int g = (int)std::max<long long>(1, std::min<long long>((waves + 3) / 4, 2048));
                k_sw_nnz<<<g, 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, B->sub, h->nfpb, h->par, B->qb, B->cb, B->bad);
                STEP_CK(hipGetLastError());
            }
            k_sw_edges<<<blocks_for(m + 1, 256), 256, 0, s>>>(m, B->rec, R.fr, reach_bp(h), B->ne, B->nx);
            STEP_CK(hipGetLastError());
            size_t tb = B->tmp_bytes;
            STEP_CK(hipcub::DeviceScan::ExclusiveSum(B->tmp, tb, B->ne, B->noff, m + 1, s));
            int total = 0;                                            // (<= n: a fragment belongs to at most one span)
            STEP_CK(hipMemcpyAsync(&total, B->noff + m, sizeof(int), hipMemcpyDeviceToHost, s));
            STEP_CK(hipStreamSynchronize(s));
            if (total > 0) {
                k_sw_mass<<<blocks_for(total, 4), 256, 0, s>>>(total, m, B->rec, B->noff, B->ne, B->nx, R.fr, h->nfpb, h->par, reach_bp(h), B->qb, B->bad);
                STEP_CK(hipGetLastError());
            }
            k_sw_out<<<blocks_for(m, 256), 256, 0, s>>>(m, B->rec, B->qb, B->cb, B->bad, B->q, B->c, B->st);
            STEP_CK(hipGetLastError());
        }
        STEP_CK(hipMemcpyAsync(q, B->q, sizeof(long long) * (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(contacts, B->c, sizeof(long long) * (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(status, B->st, (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    if (refused) return fail(h, GRAAL_E_ARG, msg);
    return score_exit(h, "graal_block_swaps", rc, nullptr, err);
}

} // extern "C"
