// junctions.h -- the likelihood each join of the current layout carries, for every junction in one pass (graal_junction_scores).
// Included by graal_hip.hip after layout_slots.h (it uses Ctx, Stat, centre_kb, rippe, to_q, WAVE_LDS_SYNC, model_math.h,
// wave_runs.h's run_head / run_tail / run_sum, score_common.h's score_entry, score_exit, STEP_CK, stream_blocks and mass_stripes, and
// layout_slots.h's LayoutSlots and slot_claim).
//
// J[f] = logL(layout) - logL(layout cut between f and next[f]), for f in a LINEAR contig with next[f] != -1, in the engine's exact
// arithmetic: pairs on one side of the cut are exactly unchanged, so only the pairs that STRADDLE the cut contribute -- they go from their cis
// price to their trans price (v_inter * norm, with the reference's trans-branch RF-count indexing under GRAAL_MODE_REF_TRANS_ACCU):
//   a contact:                  ob * (ln ex_cis - ln ex_trans), rounded to Q once per contact;
//   a fragment pair's mass:   -(sum over its sub-fragment pairs of ex_cis - ex_trans), rounded to Q once per fragment pair.
//
// Decomposition.  Number the fragments of the layout by slots: a contig's fragments are consecutive, in position order.  A straddling pair
// (x at slot i, y at slot j > i, one contig) adds its term c to D[i] and subtracts it at D[j]; the junction behind slot k is straddled by
// exactly the pairs with i <= k < j, so J = the inclusive prefix sum of D at f's slot.  Every pair adds and removes its term inside its own
// contig, so one inclusive scan over all slots is the per-contig scan (int64 sums wrap, the differences are exact).
//
// The slot numbering is layout_slots.h's, built from the layout itself: the call does not relabel.  Kernels, all on the engine's stream
// (behind any commit or relabel the host has launched):
//   slots_count (k_jn_count / scan) / k_jn_prep  -- slots, a 48-byte record per slot and a 16-byte record per sub-fragment (centre as the
//                 pricing has it);
//   k_jn_nnz   -- streams the row-sorted COO list, 64 consecutive contacts per wave; a wave without a term moves on; else terms are summed
//                 per run of equal slots inside the wave (a segmented shuffle scan) and only a run's last lane touches D: a row's contacts
//                 share its slot, so the row side costs about one atomic per row and wave; the column side one per run of equal column
//                 slots;
//   k_jn_mass  -- k_full_mass_t's tiling: a wave's lanes are 64 consecutive slots x, the slots y behind them staged in LDS 64 at a time, S waves
//                 per x tile.  Lane l visits the staged y's in the order l, l+1, ... (mod 64), so at every step the 64 lanes hold 64 different
//                 columns: the column sums of a tile are kept in LDS without atomics, then one device atomic per tile column, and one per
//                 row at the end;
//   k_jn_quirk -- only with GRAAL_MODE_REF_TRANS_ACCU and bins of mixed RF counts: straddling pairs beyond the window, whose trans price
//                 differs from their (v_inter) cis price by the indexing alone;
//   two inclusive scans (D, and a count of non-finite terms laid out the same way), then k_jn_out: J and a status byte per fragment.
//
// The family.  junction_boot.h and junction_gaps.h fill one D per replicate or per gap value -- a ROW -- by the same decomposition, and
// share with this file jn_contact_stream (k_jn_nnz's body over a term type), the host steps jn_reserve ... jn_finish, and for the rows
// jn_rows_batch, JnBuf's batch pair Db / Pb (one allocation: the two calls are never live together), jn_rows_scan and
// jn_zero_nonfinite.  k_jg_mass repeats k_jn_mass's walk with JG_GB values per fragment pair: one body over the number of values puts
// k_jn_mass over 72 VGPRs, an occupancy of 6 for 7 (profiles/junction_family.md), so only jn_blank and jn_mass_grid are shared there.
#pragma once

namespace {

struct JnSub { int label; float centre; int accu; int slot; };   // accu: RF count | under the trans-branch indexing << 16; slot -1: circular
struct JnFrag { int frag, start_bp, len_bp, flags; int n, a0, a1, a2; float c0, c1, c2; int last; };   // per slot; flags bit0 fwd, bit1 circ

struct JnBuf {
    int n = 0, S = 0;
    LayoutSlots L;                                         // (its tmp also serves the two inclusive scans)
    DevBuf<JnFrag> fr;
    DevBuf<JnSub> sub;
    DevBuf<long long> D, P;
    DevBuf<int> B, PB;
    size_t cells = 0;
    DevBuf<long long> Db, Pb;                              // a batch of rows (jn_rows_batch): rb * n each, D's and P's of the family's calls
    DevBuf<long long> q; DevBuf<unsigned char> st;         // the results, fragment-indexed
};

void jn_free(JnBuf* b) { delete b; }

// the record of a lane without a slot: no sub-fragment, no partner
__device__ __forceinline__ JnFrag jn_blank() { JnFrag x{}; x.last = -1; return x; }

// What k_jn_prep and k_rg_prep read of fragment f: its bp interval, orientation and topology, its Stat, and the centres of its (up to
// three) sub-fragments as the pricing has them.
struct JnLoad { Stat st; int start, len; bool fwd, circ; float c0, c1, c2; };

__device__ __forceinline__ JnLoad jn_load(SoaPtr s, const Stat* __restrict__ stat, int f)
{
    JnLoad x;
    x.st = stat[f];
    x.fwd = s.p[F_ORI][f] == 1; x.circ = s.p[F_CIRC][f] == 1;
    x.start = s.p[F_START][f]; x.len = s.p[F_LEN][f];
    x.c0 = x.st.n > 0 ? centre_kb(x.start, x.fwd, x.st, 0) : 0.0f;
    x.c1 = x.st.n > 1 ? centre_kb(x.start, x.fwd, x.st, 1) : 0.0f;
    x.c2 = x.st.n > 2 ? centre_kb(x.start, x.fwd, x.st, 2) : 0.0f;
    return x;
}

__global__ __launch_bounds__(256) void k_jn_prep(SoaPtr s, int n, const Stat* __restrict__ stat, const int* __restrict__ sub_ids,
                                                 const int* __restrict__ cnt, const int* __restrict__ base, int* __restrict__ slot_of,
                                                 JnFrag* __restrict__ fr, JnSub* __restrict__ sub, unsigned* __restrict__ err)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int slot = slot_claim(s, n, f, cnt, base, slot_of, err);
    if (slot < 0) return;
    const int c = s.p[F_IDC][f];
    const JnLoad x = jn_load(s, stat, f);
    const Stat& st = x.st;
    JnFrag r;
    r.frag = f; r.start_bp = x.start; r.len_bp = x.len; r.flags = (x.fwd ? 1 : 0) | (x.circ ? 2 : 0);
    r.n = st.n; r.a0 = st.a0; r.a1 = st.a1; r.a2 = st.a2;
    r.c0 = x.c0; r.c1 = x.c1; r.c2 = x.c2;
    r.last = base[c] + cnt[c] - 1;
    fr[slot] = r;
    int4 ids = make_int4(f, 0, 0, 1);
    if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[f];
    for (int k = 0; k < st.n; k++) {
        JnSub u;
        u.label = c;
        u.centre = sel3(r.c0, r.c1, r.c2, k);
        u.accu = stat_accu(st, k) | ((x.fwd ? stat_accu(st, k) : stat_accu(st, st.n - 1)) << 16);   // (RF counts are <= 30000)
        u.slot = x.circ ? -1 : slot;
        sub[sel3(ids.x, ids.y, ids.z, k)] = u;
    }
}

__device__ __forceinline__ void jn_bad(int* __restrict__ B, int i, int j)
{
    atomicAdd(&B[i < j ? i : j], 1);
    atomicAdd(&B[i < j ? j : i], -1);
}

// What one observed count of a contact between sub-fragments A and Bs adds to the junctions it straddles: t = ln ex_cis - ln ex_trans.
// False when the contact has no term (another contig, a ring, one fragment, or beyond the window with the same indexing).
__device__ __forceinline__ bool jn_contact_unit(const JnSub& A, const JnSub& Bs, const JnFrag* __restrict__ fr, float nfpb, const Par& par,
                                                int quirk, double& t)
{
    if (!(A.slot >= 0 && Bs.slot >= 0 && A.label == Bs.label && A.slot != Bs.slot)) return false;
    const int lo_a = A.accu & 0xffff, lo_b = Bs.accu & 0xffff;
    const int prod = lo_a * lo_b;
    int prod_t = prod;
    if (quirk && ((A.accu >> 16) != lo_a || (Bs.accu >> 16) != lo_b)) {
        const int bin_a = fr[A.slot].frag, bin_b = fr[Bs.slot].frag;
        prod_t = bin_a < bin_b ? (A.accu >> 16) * lo_b : lo_a * (Bs.accu >> 16);
    }
    const float sd = fabsf(Bs.centre - A.centre);
    // (at |d| >= d_max rippe is v_inter exactly: the cis and trans prices are the same float32 value unless the indexing differs)
    if (sd >= par.d_max && prod_t == prod && par.v_inter >= 0.0f) return false;
    const float ex = rippe(sd, par) * ((float)prod / nfpb);
    const float et = par.v_inter * ((float)prod_t / nfpb);
    t = mm_ln(ex) - mm_ln(et);
    return true;
}

// The family's contact stream: 64 consecutive contacts per wave; per contact the two records and term.setup(A, Bs, row id, column id,
// count): has it a term; a wave without one moves on; else the runs of equal row and of equal column slots once, then per row r < rows
// term.q(r) (Q_BAD: marked in B), two segmented sums and one 64-bit atomic per run tail into D[r * n + slot].
template <class Term>
__device__ __forceinline__ void jn_contact_stream(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt,
                                                  long long nnz, const JnSub* __restrict__ sub, Term term, int rows, int n,
                                                  long long* __restrict__ D, int* __restrict__ B)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {   // (wave-uniform bounds: the run sums need the whole wave)
        const long long k = k0 + lane;
        int ka = -1, kb = -1;
        bool has = false;
        if (k < nnz) {
            const int ra = row[k], cb = col[k];
            const JnSub A = sub[ra], Bs = sub[cb];
            ka = A.slot; kb = Bs.slot;
            has = term.setup(A, Bs, ra, cb, cnt[k]);
        }
        if (__ballot(has) == 0ull) continue;
        const int ha = run_head(ka), hb = run_head(kb);
        const bool ta = run_tail(ka) && ka >= 0, tb = run_tail(kb) && kb >= 0;
        const bool fwd = ka < kb;
        for (int r = 0; r < rows; r++) {
            long long c = 0;
            if (has) {
                const long long q = term.q(r);
                if (q == Q_BAD) jn_bad(B, ka, kb);
                else c = fwd ? q : -q;
            }
            const long long vr = run_sum(c, ha), vc = run_sum(-c, hb);
            long long* const Dr = D + (size_t)r * (size_t)n;
            if (ta && vr != 0) atomicAdd((unsigned long long*)&Dr[ka], (unsigned long long)vr);
            if (tb && vc != 0) atomicAdd((unsigned long long*)&Dr[kb], (unsigned long long)vc);
        }
    }
}

// the observed count times the unit term, one row
struct JnPlain {
    const JnFrag* __restrict__ fr; float nfpb; const Par& par; int quirk;
    double t = 0.0, ob = 0.0;
    __device__ __forceinline__ bool setup(const JnSub& A, const JnSub& Bs, int, int, const int& cnt)
    {
        if (!jn_contact_unit(A, Bs, fr, nfpb, par, quirk, t)) return false;
        ob = (double)__int_as_float(cnt);
        return true;
    }
    __device__ __forceinline__ long long q(int) const { return to_q(ob * t); }
};

__global__ __launch_bounds__(256) void k_jn_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt,
                                                long long nnz, const JnSub* __restrict__ sub, const JnFrag* __restrict__ fr, float nfpb, Par par,
                                                int quirk, long long* __restrict__ D, int* __restrict__ B)
{
    jn_contact_stream(row, col, cnt, nnz, sub, JnPlain{fr, nfpb, par, quirk}, 1, 0, D, B);
}

// trans price of sub-fragment pair (a, b) of fragments x, y: v_inter * norm, with the reference's indexing when `quirk` (ex_pair_ref)
__device__ __forceinline__ float jn_trans(int ax, int ay, int lx, int ly, bool fwd_x, bool fwd_y, int fx, int fy, float nfpb, const Par& par, int quirk)
{
    if (quirk) { if (fx < fy) { if (!fwd_x) ax = lx; } else if (!fwd_y) ay = ly; }
    return par.v_inter * ((float)(ax * ay) / nfpb);
}

__device__ __forceinline__ double jn_pair_mass(const JnFrag& x, const JnFrag& y, float nfpb, const Par& par, int quirk)
{
    double acc = 0.0;
    const int lx = sel3(x.a0, x.a1, x.a2, x.n - 1), ly = sel3(y.a0, y.a1, y.a2, y.n - 1);
    for (int a = 0; a < x.n; a++)
        for (int b = 0; b < y.n; b++) {
            const int ax = sel3(x.a0, x.a1, x.a2, a), ay = sel3(y.a0, y.a1, y.a2, b);
            const float norm = (float)(ax * ay) / nfpb;
            const float sd = fabsf(sel3(y.c0, y.c1, y.c2, b) - sel3(x.c0, x.c1, x.c2, a));
            const float ex = rippe(sd, par) * norm;
            acc += (double)ex - (double)jn_trans(ax, ay, lx, ly, x.flags & 1, y.flags & 1, x.frag, y.frag, nfpb, par, quirk);
        }
    return acc;
}

__global__ __launch_bounds__(256) void k_jn_mass(int n, const JnFrag* __restrict__ fr, float nfpb, Par par, int quirk, int reach_bp, int S,
                                                 long long* __restrict__ D, int* __restrict__ B)
{
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int W = blockIdx.x * 4 + wib, tile = W / S, s = W - tile * S;
    __shared__ JnFrag s_y[4][64];
    __shared__ long long s_col[4][64];
    JnFrag* const ty = s_y[wib];
    long long* const tc = s_col[wib];
    const int i = tile * 64 + lane;
    JnFrag x = jn_blank();
    if (i < n) { x = fr[i]; x.last = min(x.last, n - 1); }
    const int x_end = x.start_bp + x.len_bp;
    long long row = 0;
    tc[lane] = 0;
    bool live = i < n && !(x.flags & 2) && x.last > i;
    for (int c = s; ; c += S) {
        const int j0 = tile * 64 + 64 * c;
        if (__ballot(live && x.last >= j0) == 0ull) break;
        if (j0 + lane < n) ty[lane] = fr[j0 + lane];
        WAVE_LDS_SYNC();
        bool beyond = false;
        for (int t = 0; t < 64; t++) {
            const int jj = (lane + t) & 63, j = j0 + jj;
            if (live && j > i && j <= x.last) {               // (x.last < n)
                const JnFrag& y = ty[jj];
                if (y.start_bp - x_end > reach_bp) beyond = true;   // beyond the window: cis = trans exactly (k_jn_quirk: the indexing)
                else {
                    const long long q = to_q_fast(jn_pair_mass(x, y, nfpb, par, quirk));
                    if (q == Q_BAD) jn_bad(B, i, j);
                    else if (q != 0) { row -= q; tc[jj] += q; }
                }
            }
            WAVE_LDS_SYNC();                                  // (step t + 1's lanes read the columns step t's lanes wrote)
        }
        const long long v = tc[lane];
        if (v != 0 && j0 + lane < n) atomicAdd((unsigned long long*)&D[j0 + lane], (unsigned long long)v);
        tc[lane] = 0;
        live = live && !beyond && x.last >= j0 + 64;
        WAVE_LDS_SYNC();
    }
    if (row != 0) atomicAdd((unsigned long long*)&D[i], (unsigned long long)row);
}

// GRAAL_MODE_REF_TRANS_ACCU with bins of mixed RF counts: a reversed such bin x, paired with a later-id bin y of its (linear) contig beyond
// the window, is priced v_inter * plain norm now and with x's last RF count once the cut separates them.  One block per such bin.
__global__ __launch_bounds__(256) void k_jn_quirk(int n, const int* __restrict__ ubins, const int* __restrict__ slot_of, const JnFrag* __restrict__ fr,
                                                  float nfpb, Par par, int reach_bp, long long* __restrict__ D, int* __restrict__ B)
{
    const int xf = ubins[blockIdx.x];
    const int i = slot_of[xf];
    if (i < 0) return;
    const JnFrag x = fr[i];
    if ((x.flags & 2) || (x.flags & 1) || x.n < 1) return;
    // (the contig's slots end at x.last and share it: walk back from there)
    for (int j = min(x.last, n - 1) - (int)threadIdx.x; j >= 0; j -= (int)blockDim.x) {
        const JnFrag y = fr[j];
        if (y.last != x.last) break;                          // left the contig (slots of one contig share their last slot)
        if (j == i || y.frag < xf || y.n < 1) continue;
        const bool far = j > i ? y.start_bp - (x.start_bp + x.len_bp) > reach_bp : x.start_bp - (y.start_bp + y.len_bp) > reach_bp;
        if (!far) continue;
        double acc = 0.0;
        const int lx = sel3(x.a0, x.a1, x.a2, x.n - 1);
        for (int a = 0; a < x.n; a++)
            for (int b = 0; b < y.n; b++) {
                const int ay = sel3(y.a0, y.a1, y.a2, b);
                acc += (double)(par.v_inter * ((float)(sel3(x.a0, x.a1, x.a2, a) * ay) / nfpb)) - (double)(par.v_inter * ((float)(lx * ay) / nfpb));
            }
        const long long q = to_q(acc);
        if (q == Q_BAD) { jn_bad(B, i, j); continue; }
        if (q == 0) continue;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        atomicAdd((unsigned long long*)&D[lo], (unsigned long long)(-q));
        atomicAdd((unsigned long long*)&D[hi], (unsigned long long)q);
    }
}

__global__ void k_jn_out(SoaPtr s, int n, const int* __restrict__ slot_of, const long long* __restrict__ P, const int* __restrict__ PB,
                         long long* __restrict__ q_out, unsigned char* __restrict__ st_out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int k = slot_of[f];
    unsigned char st;
    long long q = 0;
    if (s.p[F_CIRC][f] == 1) st = GRAAL_JUNCTION_CIRCULAR;
    else if (s.p[F_NEXT][f] == -1 || k < 0) st = GRAAL_JUNCTION_END;
    else if (PB[k] != 0) st = GRAAL_JUNCTION_NONFINITE;
    else { st = GRAAL_JUNCTION_VALID; q = P[k]; }
    q_out[f] = q;
    st_out[f] = st;
}

// The steps of graal_junction_scores, each on the engine's stream; junction_boot.h and junction_gaps.h run the same ones around their own.
inline int jn_quirk(const Ctx* h) { return (h->mode & GRAAL_MODE_REF_TRANS_ACCU) ? 1 : 0; }

constexpr size_t JB_BATCH_BYTES = 256u << 20;      // rows * n * 8 bytes <= 256 MB (twice: Db and its scan Pb)
constexpr int JB_BATCH_MAX = 64;

// the rows (replicates, gap values) of one batch: as many as fit the bound, however many the call wants (a row does not depend on it)
inline int jn_rows_batch(int n) { return (int)std::max<size_t>(1, std::min<size_t>(JB_BATCH_MAX, JB_BATCH_BYTES / (sizeof(long long) * (size_t)n))); }

// The handle's JnBuf, sized to the engine's n and S; rows: how many rows the call will fill (the batch pair for min(batch, rows) of them,
// and scratch for the scan of a whole batch).
int jn_reserve(Ctx* h, int rows = 0)
{
    const int n = h->n, S = h->n_sub_total;
    if (!h->jn) h->jn = new JnBuf();
    JnBuf* J = h->jn;
    size_t b2 = 0, b3 = 0, br = 0;
    CK(hipcub::DeviceScan::InclusiveSum(nullptr, b2, J->D.p, J->P.p, n, h->stream));
    CK(hipcub::DeviceScan::InclusiveSum(nullptr, b3, J->B.p, J->PB.p, n, h->stream));
    if (rows > 0) CK(hipcub::DeviceScan::InclusiveSum(nullptr, br, J->Db.p, J->Pb.p, (int)((size_t)jn_rows_batch(n) * (size_t)n), h->stream));
    if (const int rc = slots_reserve(h, J->L, std::max(std::max(b2, b3), br))) return rc;
    if (J->n != n || J->S != S) {
        CK(group_realloc(J->n, n, J->fr, n, J->sub, std::max(S, 1), J->D, n, J->P, n, J->B, n, J->PB, n, J->q, n, J->st, n));
        J->S = S;
    }
    const size_t cells = (size_t)std::min(jn_rows_batch(n), rows) * (size_t)n;
    CK(group_grow(J->cells, cells, J->Db, cells, J->Pb, cells));
    return GRAAL_OK;
}

// D and B cleared, the slots and the records built; err: the flags of a corrupt layout (the caller leaves when they are set).
int jn_prepare(Ctx* h, JnBuf* J, unsigned& err)
{
    const int n = h->n;
    hipStream_t s = h->stream;
    LayoutSlots& L = J->L;
    int rc = GRAAL_OK;
    do {
        STEP_CK(hipMemsetAsync(J->D, 0, sizeof(long long) * (size_t)n, s));
        STEP_CK(hipMemsetAsync(J->B, 0, sizeof(int) * (size_t)n, s));
        STEP_CK(hipMemsetAsync(J->fr, 0, sizeof(JnFrag) * (size_t)n, s));   // (a slot no fragment claims -- a corrupt layout -- reads as empty)
        if ((rc = slots_count(h, L))) break;
        k_jn_prep<<<blocks_for(n, 256), 256, 0, s>>>(h->soa[h->cur], n, h->stat_frag, h->d_sub_ids, L.cnt, L.base, L.slot, J->fr, J->sub, L.err);
        STEP_CK(hipGetLastError());
        rc = slots_read_err(h, L, err);
    } while (false);
    return rc;
}

// the contacts' terms, added to D (and B)
int jn_add_contacts(Ctx* h, JnBuf* J)
{
    int rc = GRAAL_OK;
    do {
        if (h->nnz < 1) break;
        k_jn_nnz<<<stream_blocks(h->nnz), 256, 0, h->stream>>>(h->row, h->col, h->cnt, h->nnz, J->sub, J->fr, h->nfpb, h->par, jn_quirk(h), J->D, J->B);
        STEP_CK(hipGetLastError());
    } while (false);
    return rc;
}

// the launch of a mass walk (k_jn_mass, k_jg_mass): Sw waves per tile of 64 slots, four waves per block
struct JnMassGrid { int Sw, blocks; };
inline JnMassGrid jn_mass_grid(const Ctx* h)
{
    const int Sw = mass_stripes(std::min(std::max(std::max(h->max_lcont, h->lcont_bound), 1), h->n));
    return {Sw, ((h->n + 63) / 64 * Sw + 3) / 4};
}

// the mass terms, added to D (and B)
int jn_add_mass(Ctx* h, JnBuf* J)
{
    const int n = h->n, quirk = jn_quirk(h);
    hipStream_t s = h->stream;
    int rc = GRAAL_OK;
    do {
        const JnMassGrid g = jn_mass_grid(h);
        k_jn_mass<<<g.blocks, 256, 0, s>>>(n, J->fr, h->nfpb, h->par, quirk, reach_bp(h), g.Sw, J->D, J->B);
        STEP_CK(hipGetLastError());
        if (quirk && h->n_ubins) {
            k_jn_quirk<<<h->n_ubins, 256, 0, s>>>(n, h->d_ubins, J->L.slot, J->fr, h->nfpb, h->par, reach_bp(h), J->D, J->B);
            STEP_CK(hipGetLastError());
        }
    } while (false);
    return rc;
}

// D's inclusive scan into P, `rows` rows of n: every row's D sums to zero over each contig, so one scan of the concatenation is each
// row's own scan
int jn_scan(Ctx* h, JnBuf* J, const long long* D, long long* P, int rows)
{
    int rc = GRAAL_OK;
    do {
        size_t tb = J->L.tmp.count;
        STEP_CK(hipcub::DeviceScan::InclusiveSum(J->L.tmp.p, tb, D, P, (int)((size_t)rows * (size_t)h->n), h->stream));
    } while (false);
    return rc;
}
int jn_scan_d(Ctx* h, JnBuf* J, long long* P) { return jn_scan(h, J, J->D, P, 1); }             // the call's own D
int jn_rows_scan(Ctx* h, JnBuf* J, int rb) { return jn_scan(h, J, J->Db, J->Pb, rb); }           // a batch of rb rows, Db into Pb

// On the host, behind the copies: a junction that met an unrepresentable term (in the data or in a row) has no result -- zeros, as at
// ends and in rings, in every per-fragment column `cols` and in its column of the rows x n matrix `mat` (null: none).
template <class... C>
void jn_zero_nonfinite(int n, const uint8_t* status, int64_t* mat, int rows, C*... cols)
{
    for (int f = 0; f < n; f++) {
        if (status[f] != GRAAL_JUNCTION_NONFINITE) continue;
        ((cols[f] = 0), ...);
        if (mat) for (int r = 0; r < rows; r++) mat[(size_t)r * (size_t)n + f] = 0;
    }
}

// B's inclusive scan, then J and the status byte per fragment from it and from J->P, and their copies to the host queued behind
int jn_finish(Ctx* h, JnBuf* J, int64_t* q_out, uint8_t* status)
{
    const int n = h->n;
    hipStream_t s = h->stream;
    int rc = GRAAL_OK;
    do {
        size_t tb = J->L.tmp.count;
        STEP_CK(hipcub::DeviceScan::InclusiveSum(J->L.tmp.p, tb, J->B.p, J->PB.p, n, s));
        k_jn_out<<<blocks_for(n, 256), 256, 0, s>>>(h->soa[h->cur], n, J->L.slot, J->P, J->PB, J->q, J->st);
        STEP_CK(hipGetLastError());
        STEP_CK(hipMemcpyAsync(q_out, J->q, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(status, J->st, (size_t)n, hipMemcpyDeviceToHost, s));
    } while (false);
    return rc;
}

} // namespace

extern "C" {

int graal_junction_scores(graal_ctx* h, int64_t* q_out, uint8_t* status)
{
    if (!h || !q_out || !status) return GRAAL_E_ARG;
    if (const int rc = score_entry(h, "graal_junction_scores")) return rc;
    if (h->n < 1) return GRAAL_OK;
    if (const int rc = jn_reserve(h)) return rc;
    JnBuf* J = h->jn;
    int rc = GRAAL_OK;
    unsigned err = 0;
    do {
        if ((rc = jn_prepare(h, J, err)) || err) break;
        if ((rc = jn_add_contacts(h, J))) break;
        if ((rc = jn_add_mass(h, J))) break;
        if ((rc = jn_scan_d(h, J, J->P))) break;
        if ((rc = jn_finish(h, J, q_out, status))) break;
        STEP_CK(hipStreamSynchronize(h->stream));
    } while (false);
    return score_exit(h, "graal_junction_scores", rc, nullptr, err);
}

} // extern "C"
