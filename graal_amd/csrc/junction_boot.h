// junction_boot.h -- bootstrap support for every junction of the current layout, all replicates in one call (graal_junction_bootstrap).
// Included by graal_hip.hip after junctions.h (it uses JnBuf with its batch pair, the steps of graal_junction_scores, jn_contact_stream
// and JnPlain, and simulate.h's SimStream and sim_poisson).
//
// Poisson bootstrap of read pairs: in replicate r contact k with count ob_k counts ob*_{k,r} ~ Poisson(ob_k), independently.  Only the
// CONTACT part of a junction score depends on the data:
//   J*_r[f] = M[f] + sum over the contacts k that straddle the junction of to_q((double)ob*_{k,r} * (ln ex_cis,k - ln ex_trans,k)),
// M[f] the mass part (k_jn_mass, k_jn_quirk), computed once for all replicates.  Every term is rounded to Q once per (contact, replicate)
// and summed in int64: a replicate is a function of (layout, tables, parameters, contacts, seed, r) alone -- bit-identical from call to
// call, for any grid, any n_rep and any batching.
//
// RNG contract: ob*_{k,r} = sim_poisson(ob_k, SimStream(row_k, col_k, 2 | r << 8, seed)) -- Philox4x32-10 keyed by the seed, counter
// (row, col, 2 | r << 8, draw index).  The tag's low byte is 2 (the simulator draws under 0 and 1: disjoint streams under one seed).  The
// draw depends on the contact's sub-fragment ids, not on its place in the list; two list entries with the same (row, col) draw the same
// count.  A contact without a straddling term draws nothing (the generator is counter-based: nothing shifts).
//
// Kernels, on the engine's stream:
//   graal_junction_scores' own (slots, records, k_jn_mass / k_jn_quirk, then k_jn_nnz) for M's prefix and for the data's own J;
//   k_jb_nnz  -- per batch of RB replicates: junctions.h's contact stream (jn_contact_stream), the two slots and the unit term once per
//                contact, then per replicate a draw, a term and two segmented sums, one 64-bit atomic per run tail into D[r * n + slot];
//   one hipcub InclusiveSum over the RB * n entries (jn_rows_scan);
//   k_jb_fold -- one thread per slot walks the batch's replicates in order: J*_r = M's prefix + the scan; support, sum, min, max; J*_r
//                itself into the batch's rows when the caller wants the matrix.  No atomics: the order is fixed.
// Batches: RB = jn_rows_batch(n) replicates, in JnBuf's batch pair.
#pragma once

namespace {

constexpr int JB_MAX_REP = 1024;

struct JbBuf {
    int n = 0;
    DevBuf<long long> PM;                              // M's prefix, per slot
    DevBuf<long long> sum, mn, mx; DevBuf<int> sup;    // per fragment
};

void jb_free(JbBuf* b) { delete b; }

// a resampled count times the unit term, replicate r0 + r in row r (the RNG contract above)
struct JbPoisson {
    JnPlain u; unsigned long long seed; int r0;
    unsigned ra = 0, cb = 0;
    __device__ __forceinline__ bool setup(const JnSub& A, const JnSub& Bs, int ia, int ib, const int& cnt)
    {
        ra = (unsigned)ia; cb = (unsigned)ib;
        return u.setup(A, Bs, ia, ib, cnt);
    }
    __device__ __forceinline__ long long q(int r) const
    {
        SimStream st(ra, cb, 2u | ((unsigned)(r0 + r) << 8), seed);
        return to_q((double)sim_poisson(u.ob, st) * u.t);
    }
};

__global__ __launch_bounds__(256) void k_jb_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt,
                                                long long nnz, const JnSub* __restrict__ sub, const JnFrag* __restrict__ fr, float nfpb, Par par,
                                                int quirk, unsigned long long seed, int r0, int rb, int n, long long* __restrict__ D,
                                                int* __restrict__ B)
{
    jn_contact_stream(row, col, cnt, nnz, sub, JbPoisson{{fr, nfpb, par, quirk}, seed, r0}, rb, n, D, B);
}

// One thread per slot k (fragment f = fr[k].frag).  A junction is scored behind a fragment of a linear contig that is not its last;
// every other fragment gets zeros.  first: this batch begins the call (the statistics start here).  rep: J*_r per fragment, rb rows of n
// (null: the matrix is not wanted).
__global__ __launch_bounds__(256) void k_jb_fold(int n, const JnFrag* __restrict__ fr, const long long* __restrict__ PM, const long long* __restrict__ P,
                                                 int rb, int first, long long threshold, int* __restrict__ sup, long long* __restrict__ sum,
                                                 long long* __restrict__ mn, long long* __restrict__ mx, long long* __restrict__ rep)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const JnFrag x = fr[k];
    const int f = x.frag;
    const bool scored = !(x.flags & 2) && k < x.last;
    int s = 0;
    long long a = 0, lo = 0, hi = 0;
    if (!first) { s = sup[f]; a = sum[f]; lo = mn[f]; hi = mx[f]; }
    const long long m = PM[k];
    for (int r = 0; r < rb; r++) {
        long long j = 0;
        if (scored) {
            j = m + P[(size_t)r * (size_t)n + k];
            s += j > threshold ? 1 : 0;
            a += j;
            lo = (first && r == 0) ? j : min(lo, j);
            hi = (first && r == 0) ? j : max(hi, j);
        }
        if (rep) rep[(size_t)r * (size_t)n + f] = j;
    }
    sup[f] = s; sum[f] = a; mn[f] = lo; mx[f] = hi;
}

} // namespace

extern "C" {

int graal_junction_bootstrap(graal_ctx* h, uint64_t seed, int32_t n_rep, int64_t threshold_q, int64_t* q_out, uint8_t* status, int32_t* support,
                             int64_t* q_sum, int64_t* q_min, int64_t* q_max, int64_t* q_rep)
{
    if (!h || !q_out || !status || !support || !q_sum || !q_min || !q_max) return GRAAL_E_ARG;
    if (n_rep < 1 || n_rep > JB_MAX_REP) return GRAAL_E_ARG;
    if (const int rc = score_entry(h, "graal_junction_bootstrap")) return rc;
    const int n = h->n;
    if (n < 1) return GRAAL_OK;
    const int RB = jn_rows_batch(n);
    if (!h->jb) h->jb = new JbBuf();
    JbBuf* X = h->jb;
    hipStream_t s = h->stream;
    if (const int rc = jn_reserve(h, n_rep)) return rc;
    JnBuf* J = h->jn;
    CK(group_exact(X->n, (size_t)n, X->PM, n, X->sum, n, X->mn, n, X->mx, n, X->sup, n));
    int rc = GRAAL_OK;
    unsigned err = 0;
    do {
        if ((rc = jn_prepare(h, J, err)) || err) break;
        if ((rc = jn_add_mass(h, J))) break;
        if ((rc = jn_scan_d(h, J, X->PM))) break;                 // M's prefix
        if ((rc = jn_add_contacts(h, J))) break;
        if ((rc = jn_scan_d(h, J, J->P))) break;                  // the data's own J
        for (int r0 = 0; r0 < n_rep && !rc; r0 += RB) {
            const int rb = std::min(RB, (int)n_rep - r0);
            const size_t m = (size_t)rb * (size_t)n;
            STEP_CK(hipMemsetAsync(J->Db, 0, sizeof(long long) * m, s));
            if (h->nnz > 0) {
                k_jb_nnz<<<stream_blocks(h->nnz), 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, J->sub, J->fr, h->nfpb, h->par, jn_quirk(h),
                                                               (unsigned long long)seed, r0, rb, n, J->Db, J->B);
                STEP_CK(hipGetLastError());
            }
            if ((rc = jn_rows_scan(h, J, rb))) break;
            k_jb_fold<<<blocks_for(n, 256), 256, 0, s>>>(n, J->fr, X->PM, J->Pb, rb, r0 == 0 ? 1 : 0, (long long)threshold_q, X->sup, X->sum, X->mn,
                                                         X->mx, q_rep ? J->Db.p : nullptr);
            STEP_CK(hipGetLastError());
            if (q_rep) {                                          // (the next batch clears Db: the rows leave first)
                STEP_CK(hipMemcpyAsync(q_rep + (size_t)r0 * (size_t)n, J->Db, sizeof(long long) * m, hipMemcpyDeviceToHost, s));
                STEP_CK(hipStreamSynchronize(s));
            }
        }
        if (rc) break;
        if ((rc = jn_finish(h, J, q_out, status))) break;         // (behind the batches: their unrepresentable terms are in B)
        STEP_CK(hipMemcpyAsync(support, X->sup, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(q_sum, X->sum, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(q_min, X->mn, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(q_max, X->mx, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
        jn_zero_nonfinite(n, status, q_rep, n_rep, support, q_sum, q_min, q_max);
    } while (false);
    return score_exit(h, "graal_junction_bootstrap", rc, nullptr, err);
}

} // extern "C"
