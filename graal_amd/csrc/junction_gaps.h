// junction_gaps.h -- the likelihood profile of the gap at every junction of the current layout, a grid of gap values in one call
// (graal_junction_gaps).  Included by graal_hip.hip after junction_boot.h (it uses junctions.h's JnBuf with its batch pair, JnFrag /
// JnSub, the steps of graal_junction_scores, jn_contact_stream, jn_bad, jn_blank and jn_mass_grid).
//
// G[g][f] = logL(the layout with everything behind f in its contig moved gap[g] kb further) - logL(layout), for the fragments f that
// graal_junction_scores scores.  Pairs on one side of the junction are exactly unchanged; a straddling sub-fragment pair at distance
// sd = |centre_b - centre_a| goes from its cis price at sd to its cis price at sd_g = sd + gap (one float32 addition):
//   ex_0 = rippe(sd) * norm, ex_g = rippe(sd_g) * norm, norm = (float)(accu_a * accu_b) / nfpb (the plain indexing: the pair stays cis);
//   a contact:                to_q(ob * (ln ex_g - ln ex_0)), rounded once per (contact, gap);
//   a fragment pair's mass:  -to_q(sum over its sub-fragment pairs of (double)ex_g - (double)ex_0), rounded once per (fragment pair, gap),
//                             summed in jn_pair_mass's order.
// A pair with sd >= d_max is priced v_inter * norm at every gap >= 0 and has no term (k_jn_mass's window and jn_contact_unit's skip
// hold); at gap >= d_max every pair of the window is priced v_inter * norm, its trans price: G = -J of the plain indexing.  At gap 0
// every term is exactly 0.  The terms go into D by junctions.h's decomposition (added at the lower slot, removed at the upper one, one
// inclusive scan), one D per gap value as junction_boot.h keeps one per replicate.  int64 sums: bit-identical from call to call, for any
// grid and any batching of the gap values.
//
// Kernels, on the engine's stream:
//   graal_junction_scores' own (slots, records, k_jn_nnz, k_jn_mass / k_jn_quirk) for the data's own J;
//   k_jg_nnz  -- per batch of gap values: junctions.h's contact stream (jn_contact_stream); the slots, sd, norm and ln ex_0 once per
//                contact inside the window, then per gap value one rippe, one mm_ln and the stream's sums into D[g * n + slot];
//   k_jg_mass -- k_jn_mass's tiling and rotated visiting order, JG_GB gap values per launch: ex_0 once per sub-fragment pair, then the
//                JG_GB evaluations; a tile's column sums in LDS (4 * 64 * JG_GB int64), the row sums in registers;
//   one hipcub InclusiveSum over the batch's rb * n entries (every gap's D sums to zero over each contig);
//   k_jg_fold -- one thread per slot: the batch's rows of the scan into the profile G (fragment-indexed, kept on the device for the whole
//                call: n_gaps * n int64), and behind the last batch two walks over the fragment's profile in grid order: best / q_best,
//                then lo / hi.  No atomics: the order is fixed.
// Batches: jn_rows_batch(n) gap values, in JnBuf's batch pair.
#pragma once

namespace {

constexpr int JG_MAX_GAPS = 64;
constexpr int JG_GB = 8;                               // gap values per k_jg_mass launch

struct JgBuf {
    int n = 0; size_t gcells = 0;
    DevBuf<float> gap;                                 // the grid, JG_MAX_GAPS entries
    DevBuf<int> best, lo, hi; DevBuf<long long> qb;    // per fragment
    DevBuf<long long> G;                               // the profile: n_gaps * n, fragment-indexed
};

void jg_free(JgBuf* b) { delete b; }

// the observed count times ln ex_g - ln ex_0, gap value g in row g; the plain indexing, inside the window only
struct JgGap {
    float nfpb; const Par& par; const float* __restrict__ gap;
    float sd = 0.0f, norm = 0.0f;
    double ln0 = 0.0, ob = 0.0;
    __device__ __forceinline__ bool setup(const JnSub& A, const JnSub& Bs, int, int, const int& cnt)
    {
        if (!(A.slot >= 0 && Bs.slot >= 0 && A.label == Bs.label && A.slot != Bs.slot)) return false;
        sd = fabsf(Bs.centre - A.centre);
        if (!(sd < par.d_max)) return false;                  // (beyond the window: v_inter * norm at every gap, no term)
        norm = (float)((A.accu & 0xffff) * (Bs.accu & 0xffff)) / nfpb;
        ln0 = mm_ln(rippe(sd, par) * norm);
        ob = (double)__int_as_float(cnt);
        return true;
    }
    __device__ __forceinline__ long long q(int g) const
    {
        const float sdg = sd + gap[g];
        return to_q(ob * (mm_ln(rippe(sdg, par) * norm) - ln0));
    }
};

__global__ __launch_bounds__(256) void k_jg_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt,
                                                long long nnz, const JnSub* __restrict__ sub, float nfpb, Par par,
                                                const float* __restrict__ gap, int gb, int n, long long* __restrict__ D, int* __restrict__ B)
{
    jn_contact_stream(row, col, cnt, nnz, sub, JgGap{nfpb, par, gap}, gb, n, D, B);
}

// What the sub-fragment pairs of fragments x (the lower slot) and y add to the expected mass at the gb gap values: acc[g] = the sum of
// (double)ex_g - (double)ex_0 in jn_pair_mass's order.  The grid ascends: behind the first value with sd + gap >= d_max rippe is
// v_inter without another powf (its own branch).
__device__ __forceinline__ void jg_pair_mass(const JnFrag& x, const JnFrag& y, float nfpb, const Par& par, const float (&gap)[JG_GB], int gb,
                                             double (&acc)[JG_GB])
{
#pragma unroll
    for (int g = 0; g < JG_GB; g++) acc[g] = 0.0;
    for (int a = 0; a < x.n; a++)
        for (int b = 0; b < y.n; b++) {
            const float sd = fabsf(sel3(y.c0, y.c1, y.c2, b) - sel3(x.c0, x.c1, x.c2, a));
            if (sd >= par.d_max) continue;                    // ex_g = ex_0 = v_inter * norm: exactly 0 at every gap
            const float norm = (float)(sel3(x.a0, x.a1, x.a2, a) * sel3(y.a0, y.a1, y.a2, b)) / nfpb;
            const double e0 = (double)(rippe(sd, par) * norm);
#pragma unroll
            for (int g = 0; g < JG_GB; g++)
                if (g < gb) acc[g] += (double)(rippe(sd + gap[g], par) * norm) - e0;
        }
}

__global__ __launch_bounds__(256) void k_jg_mass(int n, const JnFrag* __restrict__ fr, float nfpb, Par par, int reach_bp, int S,
                                                 const float* __restrict__ gap_in, int gb, long long* __restrict__ D, int* __restrict__ B)
{
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int W = blockIdx.x * 4 + wib, tile = W / S, s = W - tile * S;
    __shared__ JnFrag s_y[4][64];
    __shared__ long long s_col[4][JG_GB][64];
    JnFrag* const ty = s_y[wib];
    long long (*const tc)[64] = s_col[wib];
    float gap[JG_GB];
    long long row[JG_GB];
#pragma unroll
    for (int g = 0; g < JG_GB; g++) { gap[g] = g < gb ? gap_in[g] : 0.0f; row[g] = 0; tc[g][lane] = 0; }
    const int i = tile * 64 + lane;
    JnFrag x = jn_blank();
    if (i < n) { x = fr[i]; x.last = min(x.last, n - 1); }
    const int x_end = x.start_bp + x.len_bp;
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
                if (y.start_bp - x_end > reach_bp) beyond = true;   // beyond the window: every sd >= d_max
                else {
                    double acc[JG_GB];
                    jg_pair_mass(x, y, nfpb, par, gap, gb, acc);
#pragma unroll
                    for (int g = 0; g < JG_GB; g++) {
                        if (g >= gb) continue;
                        const long long q = to_q_fast(acc[g]);
                        if (q == Q_BAD) jn_bad(B, i, j);
                        else if (q != 0) { row[g] -= q; tc[g][jj] += q; }
                    }
                }
            }
            WAVE_LDS_SYNC();                                  // (step t + 1's lanes read the columns step t's lanes wrote)
        }
#pragma unroll
        for (int g = 0; g < JG_GB; g++) {
            const long long v = tc[g][lane];
            if (v != 0 && g < gb && j0 + lane < n) atomicAdd((unsigned long long*)&D[(size_t)g * (size_t)n + (size_t)(j0 + lane)], (unsigned long long)v);
            tc[g][lane] = 0;
        }
        live = live && !beyond && x.last >= j0 + 64;
        WAVE_LDS_SYNC();
    }
#pragma unroll
    for (int g = 0; g < JG_GB; g++)
        if (row[g] != 0) atomicAdd((unsigned long long*)&D[(size_t)g * (size_t)n + (size_t)i], (unsigned long long)row[g]);   // (row != 0: i < n, g < gb)
}

// One thread per slot k (fragment f = fr[k].frag).  The batch's rows g0 .. g0 + rb - 1 of the profile: G[g][f] = the scan at the slot
// for a scored fragment (junction_boot.h's rule), else 0.  last: the profile is complete -- best = the grid index of the largest G (ties:
// the smallest gap), q_best = that G, lo / hi = the smallest and largest index with G >= q_best - drop_q, from a second walk over the
// fragment's own column of G (written by this very thread, in this launch and the ones before).
__global__ __launch_bounds__(256) void k_jg_fold(int n, const JnFrag* __restrict__ fr, const long long* __restrict__ P, int g0, int rb, int n_gaps,
                                                 int last, long long drop_q, long long* __restrict__ G, int* __restrict__ best,
                                                 long long* __restrict__ qb, int* __restrict__ lo, int* __restrict__ hi)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const JnFrag x = fr[k];
    const int f = x.frag;
    const bool scored = !(x.flags & 2) && k < x.last;
    for (int g = 0; g < rb; g++) G[(size_t)(g0 + g) * (size_t)n + f] = scored ? P[(size_t)g * (size_t)n + k] : 0;
    if (!last) return;
    int b = 0;
    long long q = G[f];
    for (int g = 1; g < n_gaps; g++) {
        const long long v = G[(size_t)g * (size_t)n + f];
        if (v > q) { q = v; b = g; }
    }
    int l = b, u = b;
    for (int g = 0; g < n_gaps; g++) {
        const long long v = G[(size_t)g * (size_t)n + f];
        if ((unsigned long long)q - (unsigned long long)v <= (unsigned long long)drop_q) { if (g < l) l = g; if (g > u) u = g; }   // (q >= v)
    }
    best[f] = scored ? b : 0; qb[f] = q; lo[f] = scored ? l : 0; hi[f] = scored ? u : 0;
}

} // namespace

extern "C" {

int graal_junction_gaps(graal_ctx* h, const float* gap_kb, int32_t n_gaps, int64_t drop_q, int64_t* q_out, uint8_t* status, int32_t* best,
                        int64_t* q_best, int32_t* lo, int32_t* hi, int64_t* q_gap)
{
    if (!h || !gap_kb || !q_out || !status || !best || !q_best || !lo || !hi) return GRAAL_E_ARG;
    if (n_gaps < 1 || n_gaps > JG_MAX_GAPS || drop_q < 0) return GRAAL_E_ARG;
    for (int g = 0; g < n_gaps; g++)                          // finite, gap[0] >= 0, strictly ascending
        if (!std::isfinite(gap_kb[g]) || !(gap_kb[g] > (g ? gap_kb[g - 1] : -1.0f)) || gap_kb[g] < 0.0f) return GRAAL_E_ARG;
    if (const int rc = score_entry(h, "graal_junction_gaps")) return rc;
    const int n = h->n;
    if (n < 1) return GRAAL_OK;
    const int RB = jn_rows_batch(n);
    if (!h->jg) h->jg = new JgBuf();
    JgBuf* X = h->jg;
    hipStream_t s = h->stream;
    const size_t gcells = (size_t)n_gaps * (size_t)n;
    if (const int rc = jn_reserve(h, n_gaps)) return rc;
    JnBuf* J = h->jn;
    CK(group_exact(X->n, (size_t)n, X->best, n, X->lo, n, X->hi, n, X->qb, n));
    CK(X->gap.reserve_exact(JG_MAX_GAPS));
    CK(group_grow(X->gcells, gcells, X->G, gcells));
    int rc = GRAAL_OK;
    unsigned err = 0;
    do {
        if ((rc = jn_prepare(h, J, err)) || err) break;
        if ((rc = jn_add_contacts(h, J))) break;
        if ((rc = jn_add_mass(h, J))) break;
        if ((rc = jn_scan_d(h, J, J->P))) break;                  // the data's own J
        STEP_CK(hipMemcpyAsync(X->gap, gap_kb, sizeof(float) * (size_t)n_gaps, hipMemcpyHostToDevice, s));
        const JnMassGrid mg = jn_mass_grid(h);
        for (int g0 = 0; g0 < n_gaps && !rc; g0 += RB) {
            const int rb = std::min(RB, (int)n_gaps - g0);
            const size_t m = (size_t)rb * (size_t)n;
            STEP_CK(hipMemsetAsync(J->Db, 0, sizeof(long long) * m, s));
            if (h->nnz > 0) {
                k_jg_nnz<<<stream_blocks(h->nnz), 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, J->sub, h->nfpb, h->par, X->gap.p + g0, rb, n,
                                                               J->Db, J->B);
                STEP_CK(hipGetLastError());
            }
            for (int g1 = 0; g1 < rb && !rc; g1 += JG_GB) {
                k_jg_mass<<<mg.blocks, 256, 0, s>>>(n, J->fr, h->nfpb, h->par, reach_bp(h), mg.Sw, X->gap.p + g0 + g1, std::min(JG_GB, rb - g1),
                                                    J->Db.p + (size_t)g1 * (size_t)n, J->B);
                STEP_CK(hipGetLastError());
            }
            if (rc) break;
            if ((rc = jn_rows_scan(h, J, rb))) break;
            k_jg_fold<<<blocks_for(n, 256), 256, 0, s>>>(n, J->fr, J->Pb, g0, rb, n_gaps, g0 + rb >= n_gaps ? 1 : 0, (long long)drop_q, X->G,
                                                         X->best, X->qb, X->lo, X->hi);
            STEP_CK(hipGetLastError());
        }
        if (rc) break;
        if ((rc = jn_finish(h, J, q_out, status))) break;         // (behind the batches: their unrepresentable terms are in B)
        STEP_CK(hipMemcpyAsync(best, X->best, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(q_best, X->qb, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(lo, X->lo, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(hi, X->hi, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
        if (q_gap) STEP_CK(hipMemcpyAsync(q_gap, X->G, sizeof(long long) * gcells, hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
        jn_zero_nonfinite(n, status, q_gap, n_gaps, best, q_best, lo, hi);
    } while (false);
    return score_exit(h, "graal_junction_gaps", rc, nullptr, err);
}

} // extern "C"
