// flips.h -- the likelihood each in-place reversal of a block of fragments would add, for a caller's set of disjoint blocks in one pass
// (graal_block_flips).  Included by graal_hip.hip after links.h (it uses LayoutRecs with recs_reserve / recs_build, the records LnFrag /
// LnCtg, ln_run_sum, ln_block_add, ln_mirror_q, and score_common.h's score_entry, score_exit, STEP_CK and free_null).
//
// Block k = the fragments of one contig at positions pos[first[k]] .. pos[last[k]].  The flipped layout reverses the block inside its bp
// interval [s0, e1): a fragment (start s, length l) goes to s0 + e1 - (s + l), its ori changes sign, everything else keeps every field;
// the float32 centres through centre_kb from the integer starts in the new orientation.  F(k) = logL(flipped) - logL(current) in the
// exact arithmetic with the roundings of junctions.h / links.h: pairs inside the block and pairs outside it count as unchanged; every
// sub-fragment pair of (block) x (rest of the contig) moves from its cis price to its cis price in the flipped layout
//   a contact:                ob * (ln ex_new - ln ex_old), rounded to Q once per contact (0 where the two prices are the same float32);
//   a fragment pair's mass:   -(sum over its sub-fragment pairs of ex_new - ex_old), the block's fragment outer, rounded to Q once.
// A fragment x of the block lies dL = s - s0 behind the block's left boundary and dR = e1 - (s + l) before its right one; a flank fragment
// y lies g bp outside the boundary it faces.  The gap between them is dL + g on one side of the flip and dR + g on the other (which is
// which depends on the flank), so the pair is beyond the window both times -- priced v_inter * norm twice, difference exactly 0 --
// iff min(dL, dR) + g > reach_bp.  Only the block's fragments within reach of either boundary and the flank fragments within reach of a
// boundary take part: at most about (2w) x (2w) fragment pairs per block, however long the block.
// Under GRAAL_MODE_REF_TRANS_ACCU the flip changes the orientation of the block's bins of mixed RF counts, and with it the trans price of
// every pair (such a bin x, a higher-id bin y of ANOTHER contig): links.h's mirror term, summed per block (cis prices do not use the
// indexing, so nothing else changes inside the contig).
//
// Every fragment belongs to at most one block, so a contact feeds at most two sums and the list is streamed once; no candidate table.
// Kernels, all on the engine's stream:
//   k_jn_count / scan / k_ln_prep (recs_build) -- slots and per-slot records, as for links and insertions;
//   k_fl_gather -- per block of the caller: the slots of its two fragments, their labels, its bp interval, its contig's slots.  The host
//                 validates from these (two contigs, reversed order, overlap: an ordered set of the blocks so far), sets aside the blocks that are a
//                 whole contig or lie in a ring, and uploads the others sorted by first slot;
//   k_fl_sub    -- per fragment: its block (binary search over the sorted blocks) and, per sub-fragment, a 32-byte record with its current
//                 and its flipped centre (well defined: a fragment belongs to at most one block);
//   k_fl_nnz    -- streams the contact list once, 64 consecutive contacts per wave.  A contact of one contig whose sides have different
//                 blocks (one may be none) is priced for side A's block with A's flipped centre against B's current one, and the same
//                 for side B: two blocks each receive their own term, priced with only that block flipped.  Sums per run of equal block
//                 inside the wave (ln_run_sum) before the atomics; the mirror's contact part and the contact counts ride along;
//   k_fl_edges / scan / k_fl_mass -- work units (block, one fragment of the block within reach of a boundary) from a prefix sum, a wave
//                 per unit; its lanes walk the two flanks outwards 64 fragments at a time (each flank record is read once, by one lane:
//                 nothing to stage) and stop when a whole step is out of reach; one atomic per wave;
//   k_fl_mirror -- only with the mode flag and mixed bins: one workgroup per mixed bin, links' per-bin term, added to the bin's block;
//   k_fl_out    -- status and q per block, in the caller's order.
#pragma once

namespace {

struct FlSub { float c_old, c_new; int label, blk, frag, acc, meta, pad; };   // acc: RF count | the bin's last RF count << 16; meta: fwd | mixed << 1
struct FlInfo { int slot_f, slot_l, lab_f, lab_l, s0, e1, cfirst, ccnt, circ, pad; };   // per block of the caller
struct FlBlk { int s0, e1, first, last, cfirst, clast, id, pad; };   // the scored blocks, sorted by first slot; id: the caller's index

struct FlBuf {
    LayoutRecs R;
    FlSub* sub = nullptr; int* blk = nullptr; int n = 0, S = 0;       // per sub-fragment; the block of every slot (or -1)
    int *first = nullptr, *last = nullptr; FlInfo* info = nullptr; FlBlk* rec = nullptr;
    long long *qb = nullptr, *cb = nullptr, *q = nullptr, *c = nullptr; int *bad = nullptr, *ne = nullptr, *nl = nullptr, *noff = nullptr;
    unsigned char* st = nullptr;
    void* tmp = nullptr; size_t tmp_bytes = 0;
    size_t bcap = 0;                                                  // blocks the per-block arrays hold
};

void fl_free_blocks(FlBuf* b)
{
    free_null({(void**)&b->first, (void**)&b->last, (void**)&b->info, (void**)&b->rec, (void**)&b->qb, (void**)&b->cb, (void**)&b->q, (void**)&b->c,
               (void**)&b->bad, (void**)&b->ne, (void**)&b->nl, (void**)&b->noff, (void**)&b->st, &b->tmp});
    b->bcap = 0; b->tmp_bytes = 0;
}

void fl_free_subs(FlBuf* b)
{
    free_null({(void**)&b->sub, (void**)&b->blk});
    b->n = 0; b->S = 0;
}

void fl_free(FlBuf* b)
{
    if (!b) return;
    recs_free(b->R); fl_free_subs(b); fl_free_blocks(b);
    delete b;
}

__global__ void k_fl_gather(int nb, int n, const int* __restrict__ first, const int* __restrict__ last, const int* __restrict__ slot_of,
                            const int* __restrict__ lab, const LnFrag* __restrict__ fr, const LnCtg* __restrict__ ctg, FlInfo* __restrict__ info)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nb) return;
    FlInfo r = {-1, -1, -1, -1, 0, 0, 0, 0, 0, 0};
    const int f = first[k], l = last[k];                             // (in [0, n): the host checked)
    const int sf = slot_of[f], sl = slot_of[l];
    if (sf >= 0 && sf < n && sl >= 0 && sl < n) {
        r.slot_f = sf; r.slot_l = sl; r.lab_f = lab[f]; r.lab_l = lab[l];
        const LnFrag a = fr[sf], b = fr[sl];
        r.s0 = a.start; r.e1 = b.start + b.len;
        const LnCtg c = ctg[r.lab_f];
        r.cfirst = c.first; r.ccnt = c.cnt; r.circ = c.elig ? 0 : 1;   // (records built with min_frags 1: elig = linear)
    }
    info[k] = r;
}

// the scored block that holds `slot`, or -1: the last block that starts at or before it, if it reaches that far
__device__ __forceinline__ int fl_block_of(const FlBlk* __restrict__ rec, int m, int slot)
{
    int lo = 0, hi = m;                                              // first block with .first > slot
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rec[mid].first <= slot) lo = mid + 1; else hi = mid;
    }
    return (lo > 0 && slot <= rec[lo - 1].last) ? lo - 1 : -1;
}

__global__ __launch_bounds__(256) void k_fl_sub(int n, int m, const FlBlk* __restrict__ rec, const int* __restrict__ slot_of, const int* __restrict__ lab,
                                                const LnFrag* __restrict__ fr, const int* __restrict__ sub_ids, int* __restrict__ blk,
                                                FlSub* __restrict__ sub)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int slot = slot_of[f];
    if (slot < 0 || slot >= n) return;                               // (a corrupt layout: refused before anything reads the records)
    const LnFrag x = fr[slot];
    const int j = fl_block_of(rec, m, slot);
    blk[slot] = j;
    int ns = x.start;
    bool nf = x.fwd != 0;
    if (j >= 0) { const FlBlk b = rec[j]; ns = (int)((long long)b.s0 + b.e1 - ((long long)x.start + x.len)); nf = !nf; }
    const int last = stat_accu(x.st, x.st.n - 1);
    int4 ids = make_int4(f, 0, 0, 1);
    if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[f];
    for (int k = 0; k < x.st.n; k++) {
        FlSub u;
        u.c_old = centre_kb(x.start, x.fwd != 0, x.st, k);
        u.c_new = j >= 0 ? centre_kb(ns, nf, x.st, k) : u.c_old;
        u.label = lab[f]; u.blk = j; u.frag = f; u.pad = 0;
        u.acc = stat_accu(x.st, k) | (last << 16);                   // (RF counts are <= 30000)
        u.meta = (x.fwd ? 1 : 0) | (stat_uniform(x.st) ? 0 : 2);
        sub[sel3(ids.x, ids.y, ids.z, k)] = u;
    }
}

// a contact of a block's sub-fragment whose centre the flip moves to distance sd_new from its partner: the term, the count inside the window
__device__ __forceinline__ void fl_contact(float sd_new, float ex_old, float norm, double ob, const Par& par, long long& q, long long& c, long long& bad)
{
    if (sd_new < par.d_max) c = (long long)llrint(ob);
    const float ex_new = rippe(sd_new, par) * norm;
    if (ex_new == ex_old) return;                                    // (both beyond the window, or the distance did not change)
    const long long t = to_q(ob * (mm_ln(ex_new) - mm_ln(ex_old)));
    if (t == Q_BAD) bad = 1; else q = t;
}

__device__ __forceinline__ void fl_add(unsigned long long key, long long q, long long c, long long bad, long long* __restrict__ qb,
                                       long long* __restrict__ cb, int* __restrict__ badb)
{
    bool tail;
    ln_run_sum(key, q, c, bad, tail);
    if (tail && key != LN_EMPTY) {
        if (q != 0) atomicAdd((unsigned long long*)&qb[key], (unsigned long long)q);
        if (c != 0) atomicAdd((unsigned long long*)&cb[key], (unsigned long long)c);
        if (bad != 0) atomicAdd(&badb[key], (int)bad);
    }
}

__global__ __launch_bounds__(256) void k_fl_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt, long long nnz,
                                                const FlSub* __restrict__ sub, float nfpb, Par par, int quirk, long long* __restrict__ qb,
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
            const FlSub A = sub[row[k]], B = sub[col[k]];
            const double ob = (double)__int_as_float(cnt[k]);
            const int own_a = A.acc & 0xffff, own_b = B.acc & 0xffff;
            if (A.label == B.label) {
                if (A.blk != B.blk) {                                // (sub-fragments of one bin share their block)
                    const float norm = (float)(own_a * own_b) / nfpb;
                    const float ex_old = rippe(fabsf(B.c_old - A.c_old), par) * norm;
                    if (A.blk >= 0) { ka = (unsigned long long)A.blk; fl_contact(fabsf(B.c_old - A.c_new), ex_old, norm, ob, par, qa, ca, ba); }
                    if (B.blk >= 0) { kb = (unsigned long long)B.blk; fl_contact(fabsf(B.c_new - A.c_old), ex_old, norm, ob, par, qc, cc, bc); }
                }
            } else if (quirk) {                                      // the mirror's contact part: the lower-id bin's orientation picks the indexing
                const bool a_low = A.frag < B.frag;
                const FlSub& lo = a_low ? A : B;
                if (lo.blk >= 0 && (lo.meta & 2)) {
                    const int own_l = lo.acc & 0xffff, last_l = lo.acc >> 16, other = a_low ? own_b : own_a;
                    const bool fwd = lo.meta & 1;
                    const int prod_t = (fwd ? own_l : last_l) * other, prod_f = (fwd ? last_l : own_l) * other;
                    if (prod_f != prod_t) {
                        const float et = par.v_inter * ((float)prod_t / nfpb), ef = par.v_inter * ((float)prod_f / nfpb);
                        const long long t = to_q(ob * (mm_ln(ef) - mm_ln(et)));
                        if (a_low) { ka = (unsigned long long)A.blk; if (t == Q_BAD) ba = 1; else qa = t; }
                        else { kb = (unsigned long long)B.blk; if (t == Q_BAD) bc = 1; else qc = t; }
                    }
                }
            }
        }
        if (__ballot(ka != LN_EMPTY) != 0ull) fl_add(ka, qa, ca, ba, qb, cb, badb);
        if (__ballot(kb != LN_EMPTY) != 0ull) fl_add(kb, qc, cc, bc, qb, cb, badb);
    }
}

// the fragments of a block within reach of a boundary: nl from its first slot on (dL <= reach), nr up to its last (dR <= reach); all of
// them when the two runs meet.  One thread per block; starts grow with the slot, so both counts come from binary searches.
__global__ void k_fl_edges(int m, const FlBlk* __restrict__ rec, const LnFrag* __restrict__ fr, int reach_bp, int* __restrict__ ne, int* __restrict__ nl)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > m) return;
    if (j == m) { ne[m] = 0; return; }                               // (the scan's last entry: the total)
    const FlBlk b = rec[j];
    const int len = b.last - b.first + 1;
    int lo = 0, hi = len;                                            // first u with dL > reach
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)fr[b.first + mid].start - b.s0 <= reach_bp) lo = mid + 1; else hi = mid;
    }
    const int n_left = lo;
    lo = 0; hi = len;                                                // first u (counted from the last slot down) with dR > reach
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const LnFrag x = fr[b.last - mid];
        if ((long long)b.e1 - ((long long)x.start + x.len) <= reach_bp) lo = mid + 1; else hi = mid;
    }
    const int n_right = lo;
    if ((long long)n_left + n_right >= len) { ne[j] = len; nl[j] = len; }
    else { ne[j] = n_left + n_right; nl[j] = n_left; }
}

// mass term of the block's fragment x (current centres xo, flipped centres xn) and flank fragment y: -(sum of ex_new - ex_old), x outer
__device__ __forceinline__ long long fl_pair_q(const LnFrag& x, float xo0, float xo1, float xo2, float xn0, float xn1, float xn2, const LnFrag& y,
                                               float nfpb, const Par& par)
{
    double acc = 0.0;
    for (int a = 0; a < x.st.n; a++) {
        const int ax = stat_accu(x.st, a);
        const float co = sel3(xo0, xo1, xo2, a), cn = sel3(xn0, xn1, xn2, a);
        for (int b = 0; b < y.st.n; b++) {
            const float norm = (float)(ax * stat_accu(y.st, b)) / nfpb;
            const float cy = centre_kb(y.start, y.fwd != 0, y.st, b);
            acc += ((double)(rippe(fabsf(cy - cn), par) * norm) - (double)(rippe(fabsf(cy - co), par) * norm));   // (new - old is exact in float64)
        }
    }
    return to_q_fast(acc);
}

// the unit's block: the last j with noff[j] <= W (every block has at least one unit)
__device__ __forceinline__ int fl_block_of_unit(const int* __restrict__ noff, int m, int W)
{
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (noff[mid] <= W) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_fl_mass(int total, int m, const FlBlk* __restrict__ rec, const int* __restrict__ noff, const int* __restrict__ ne,
                                                 const int* __restrict__ nl, const LnFrag* __restrict__ fr, float nfpb, Par par, int reach_bp,
                                                 long long* __restrict__ qb, int* __restrict__ badb)
{
    const int W = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (W >= total) return;                                          // (wave-uniform)
    const int lane = threadIdx.x & 63;
    const int j = fl_block_of_unit(noff, m, W);
    const int u = W - noff[j];
    if (u < 0 || u >= ne[j]) return;
    const FlBlk b = rec[j];
    const int left = nl[j];
    const LnFrag x = fr[u < left ? b.first + u : b.last - (u - left)];
    const int dl = x.start - b.s0, dr = (int)((long long)b.e1 - ((long long)x.start + x.len));
    const int budget = reach_bp - min(dl, dr);                       // a flank fragment takes part while its gap to the boundary is <= this
    const int ns = (int)((long long)b.s0 + b.e1 - ((long long)x.start + x.len));   // (the sum of two offsets may pass 2^31)
    const bool fo = x.fwd != 0;
    const float xo0 = centre_kb(x.start, fo, x.st, 0), xo1 = x.st.n > 1 ? centre_kb(x.start, fo, x.st, 1) : 0.0f,
                xo2 = x.st.n > 2 ? centre_kb(x.start, fo, x.st, 2) : 0.0f;
    const float xn0 = centre_kb(ns, !fo, x.st, 0), xn1 = x.st.n > 1 ? centre_kb(ns, !fo, x.st, 1) : 0.0f,
                xn2 = x.st.n > 2 ? centre_kb(ns, !fo, x.st, 2) : 0.0f;
    long long sum = 0, nb = 0;
    if (budget >= 0) {
        for (int side = 0; side < 2; side++)
            for (int t = lane; ; t += 64) {                          // outwards from the boundary: the gap only grows
                const int i = side == 0 ? b.first - 1 - t : b.last + 1 + t;
                bool in = side == 0 ? i >= b.cfirst : i <= b.clast;
                LnFrag y;
                if (in) {
                    y = fr[i];
                    const long long g = side == 0 ? (long long)b.s0 - ((long long)y.start + y.len) : (long long)y.start - b.e1;
                    in = g <= budget;
                }
                if (__ballot(in) == 0ull) break;
                if (in) {
                    const long long q = fl_pair_q(x, xo0, xo1, xo2, xn0, xn1, xn2, y, nfpb, par);
                    if (q == Q_BAD) nb++; else sum -= q;
                }
            }
    }
    ln_block_add(sum, nb, &qb[j], &badb[j]);
}

// the mirror's mass part: one workgroup per mixed bin x of a scored block, against every higher-id bin of another contig (k_ln_mirror's term)
__global__ __launch_bounds__(256) void k_fl_mirror(int n, const int* __restrict__ ubins, const int* __restrict__ slot_of, const int* __restrict__ lab,
                                                   const int* __restrict__ blk, const LnFrag* __restrict__ fr, float nfpb, Par par,
                                                   long long* __restrict__ qb, int* __restrict__ badb)
{
    const int xf = ubins[blockIdx.x];
    if (xf < 0 || xf >= n) return;
    const int sx = slot_of[xf];
    if (sx < 0 || sx >= n) return;
    const int j = blk[sx];
    if (j < 0) return;
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

__global__ void k_fl_out(int m, const FlBlk* __restrict__ rec, const long long* __restrict__ qb, const long long* __restrict__ cb,
                         const int* __restrict__ badb, long long* __restrict__ q, long long* __restrict__ c, unsigned char* __restrict__ st)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int id = rec[j].id;
    const bool bad = badb[j] != 0;
    st[id] = bad ? GRAAL_FLIP_NONFINITE : GRAAL_FLIP_VALID;
    q[id] = bad ? 0 : qb[j];
    c[id] = cb[j];
}

} // namespace

extern "C" {

int graal_block_flips(graal_ctx* h, int32_t n_blocks, const int32_t* first, const int32_t* last, int64_t* q, int64_t* contacts, uint8_t* status)
{
    if (!h) return GRAAL_E_ARG;
    if (n_blocks < 0 || (n_blocks > 0 && (!first || !last || !q || !contacts || !status)))
        return fail(h, GRAAL_E_ARG, "graal_block_flips: n_blocks < 0 or a null array");
    if (const int rc = score_entry(h, "graal_block_flips")) return rc;
    if (n_blocks == 0) return GRAAL_OK;
    const int n = h->n, S = h->n_sub_total, nb = n_blocks;
    char msg[240];
    for (int k = 0; k < nb; k++)
        if (first[k] < 0 || first[k] >= n || last[k] < 0 || last[k] >= n) {
            snprintf(msg, sizeof msg, "graal_block_flips: block %d: fragment index out of range (%d, %d; %d fragments)", k, first[k], last[k], n);
            return fail(h, GRAAL_E_ARG, msg);
        }
    if (!h->fl) h->fl = new FlBuf();
    FlBuf* B = h->fl;
    LayoutRecs& R = B->R;
    hipStream_t s = h->stream;
    if (const int rc = recs_reserve(h, R)) return rc;
    if (B->n != n || B->S != S) {                                     // (B->n stays 0 until both are allocated)
        fl_free_subs(B);
        CK(hipMalloc(&B->sub, sizeof(FlSub) * (size_t)std::max(S, 1)));
        CK(hipMalloc(&B->blk, sizeof(int) * (size_t)n));
        B->n = n; B->S = S;
    }
    if ((size_t)nb > B->bcap) {                                       // (grows to the largest call; bcap stays 0 until the set is allocated)
        fl_free_blocks(B);
        const size_t cap = (size_t)nb + 1;
        CK(hipMalloc(&B->first, sizeof(int) * cap));
        CK(hipMalloc(&B->last, sizeof(int) * cap));
        CK(hipMalloc(&B->info, sizeof(FlInfo) * cap));
        CK(hipMalloc(&B->rec, sizeof(FlBlk) * cap));
        CK(hipMalloc(&B->qb, sizeof(long long) * cap));
        CK(hipMalloc(&B->cb, sizeof(long long) * cap));
        CK(hipMalloc(&B->q, sizeof(long long) * cap));
        CK(hipMalloc(&B->c, sizeof(long long) * cap));
        CK(hipMalloc(&B->bad, sizeof(int) * cap));
        CK(hipMalloc(&B->ne, sizeof(int) * cap));
        CK(hipMalloc(&B->nl, sizeof(int) * cap));
        CK(hipMalloc(&B->noff, sizeof(int) * cap));
        CK(hipMalloc(&B->st, cap));
        size_t tb = 0;
        CK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, B->ne, B->noff, (int)cap, s));
        CK(hipMalloc(&B->tmp, tb));
        B->tmp_bytes = tb;
        B->bcap = (size_t)nb;
    }
    const int quirk = (h->mode & GRAAL_MODE_REF_TRANS_ACCU) ? 1 : 0;
    int rc = GRAAL_OK;
    unsigned err = 0;
    bool refused = false;
    std::vector<FlInfo> info((size_t)nb);
    std::vector<FlBlk> rec;
    std::vector<unsigned char> st((size_t)nb);
    do {
        if ((rc = recs_build(h, R, 1))) break;
        STEP_CK(hipMemcpyAsync(B->first, first, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, s));
        STEP_CK(hipMemcpyAsync(B->last, last, sizeof(int) * (size_t)nb, hipMemcpyHostToDevice, s));
        k_fl_gather<<<blocks_for(nb, 256), 256, 0, s>>>(nb, n, B->first, B->last, R.slot, R.lab, R.fr, R.ctg, B->info);
        STEP_CK(hipGetLastError());
        STEP_CK(hipMemcpyAsync(&err, R.err, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(info.data(), B->info, sizeof(FlInfo) * (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
        if (err) break;   // (a corrupt layout: the slots are not to be trusted, nothing reads them)
        // ---- validation: the first offending block, by the caller's numbering
        int off = nb;
        const char* what = nullptr;
        // (overlap: the blocks enter an ordered set in the caller's order; those already in it are pairwise disjoint, so the first block
        // that meets one of its two neighbours there is the first that overlaps an earlier block)
        std::map<int, int> by_first;                                  // first slot -> last slot
        for (int k = 0; k < nb && off == nb; k++) {
            const FlInfo& I = info[(size_t)k];
            if (I.slot_f < 0) { off = k; what = "a fragment without a slot"; }
            else if (I.lab_f != I.lab_l) { off = k; what = "first and last lie on two contigs"; }
            else if (I.slot_f > I.slot_l) { off = k; what = "last lies before first"; }
            else {
                auto nx = by_first.lower_bound(I.slot_f);             // the first block that starts at or behind this one
                bool hit = nx != by_first.end() && nx->first <= I.slot_l;
                if (!hit && nx != by_first.begin()) hit = std::prev(nx)->second >= I.slot_f;
                if (hit) { off = k; what = "overlaps an earlier block"; }
                else by_first.emplace(I.slot_f, I.slot_l);
            }
        }
        if (off != nb) {
            snprintf(msg, sizeof msg, "graal_block_flips: block %d (fragments %d .. %d): %s", off, first[off], last[off], what);
            refused = true;
            break;
        }
        std::vector<int> order((size_t)nb);
        for (int k = 0; k < nb; k++) order[(size_t)k] = k;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return info[(size_t)a].slot_f < info[(size_t)b].slot_f; });
        // ---- the scored blocks, sorted by first slot; the others have their status already
        for (int i = 0; i < nb; i++) {
            const int k = order[(size_t)i];
            const FlInfo& I = info[(size_t)k];
            if (I.circ) { st[(size_t)k] = GRAAL_FLIP_CIRCULAR; continue; }
            if (I.slot_f == I.cfirst && I.slot_l == I.cfirst + I.ccnt - 1) { st[(size_t)k] = GRAAL_FLIP_WHOLE; continue; }
            st[(size_t)k] = GRAAL_FLIP_VALID;
            rec.push_back(FlBlk{I.s0, I.e1, I.slot_f, I.slot_l, I.cfirst, I.cfirst + I.ccnt - 1, k, 0});
        }
        const int m = (int)rec.size();
        STEP_CK(hipMemsetAsync(B->q, 0, sizeof(long long) * (size_t)nb, s));
        STEP_CK(hipMemsetAsync(B->c, 0, sizeof(long long) * (size_t)nb, s));
        STEP_CK(hipMemcpyAsync(B->st, st.data(), (size_t)nb, hipMemcpyHostToDevice, s));
        if (m > 0) {
            STEP_CK(hipMemcpyAsync(B->rec, rec.data(), sizeof(FlBlk) * (size_t)m, hipMemcpyHostToDevice, s));
            STEP_CK(hipMemsetAsync(B->qb, 0, sizeof(long long) * (size_t)m, s));
            STEP_CK(hipMemsetAsync(B->cb, 0, sizeof(long long) * (size_t)m, s));
            STEP_CK(hipMemsetAsync(B->bad, 0, sizeof(int) * (size_t)m, s));
            STEP_CK(hipMemsetAsync(B->blk, 0xff, sizeof(int) * (size_t)n, s));
            k_fl_sub<<<blocks_for(n, 256), 256, 0, s>>>(n, m, B->rec, R.slot, R.lab, R.fr, h->d_sub_ids, B->blk, B->sub);
            STEP_CK(hipGetLastError());
            if (h->nnz > 0) {
                const long long waves = (h->nnz + 63) / 64;
                const int g = (int)std::max<long long>(1, std::min<long long>((waves + 3) / 4, 2048));
                k_fl_nnz<<<g, 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, B->sub, h->nfpb, h->par, quirk, B->qb, B->cb, B->bad);
                STEP_CK(hipGetLastError());
            }
            k_fl_edges<<<blocks_for(m + 1, 256), 256, 0, s>>>(m, B->rec, R.fr, reach_bp(h), B->ne, B->nl);
            STEP_CK(hipGetLastError());
            size_t tb = B->tmp_bytes;
            STEP_CK(hipcub::DeviceScan::ExclusiveSum(B->tmp, tb, B->ne, B->noff, m + 1, s));
            int total = 0;                                            // (<= n: a fragment belongs to at most one block)
            STEP_CK(hipMemcpyAsync(&total, B->noff + m, sizeof(int), hipMemcpyDeviceToHost, s));
            STEP_CK(hipStreamSynchronize(s));
            if (total > 0) {
                k_fl_mass<<<blocks_for(total, 4), 256, 0, s>>>(total, m, B->rec, B->noff, B->ne, B->nl, R.fr, h->nfpb, h->par, reach_bp(h), B->qb, B->bad);
                STEP_CK(hipGetLastError());
            }
            if (quirk && h->n_ubins) {
                k_fl_mirror<<<h->n_ubins, 256, 0, s>>>(n, h->d_ubins, R.slot, R.lab, B->blk, R.fr, h->nfpb, h->par, B->qb, B->bad);
                STEP_CK(hipGetLastError());
            }
            k_fl_out<<<blocks_for(m, 256), 256, 0, s>>>(m, B->rec, B->qb, B->cb, B->bad, B->q, B->c, B->st);
            STEP_CK(hipGetLastError());
        }
        STEP_CK(hipMemcpyAsync(q, B->q, sizeof(long long) * (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(contacts, B->c, sizeof(long long) * (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(status, B->st, (size_t)nb, hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    if (refused) return fail(h, GRAAL_E_ARG, msg);
    return score_exit(h, "graal_block_flips", rc, nullptr, err);
}

} // extern "C"
