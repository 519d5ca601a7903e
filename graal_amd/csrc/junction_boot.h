// junction_boot.h -- bootstrap support for every junction of the current layout, all replicates in one call (graal_junction_bootstrap).
// Included by graal_hip.hip after junctions.h (it uses JnBuf and the steps of graal_junction_scores, jn_contact_unit and jn_bad, and
// simulate.h's SimStream and sim_poisson).
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
//   k_jb_nnz  -- per batch of RB replicates: streams the row-sorted list, 64 consecutive contacts per wave; the two slots and the unit
//                term once per contact; a wave without a term moves on; else the heads of the runs of equal row slots and of equal column
//                slots once, then per replicate a draw, a term and two segmented sums, one 64-bit atomic per run tail into D[r * n + slot];
//   one hipcub InclusiveSum over the RB * n entries: every replicate's D sums to zero over each contig, so the scan of the concatenation
//                is each replicate's own scan;
//   k_jb_fold -- one thread per slot walks the batch's replicates in order: J*_r = M's prefix + the scan; support, sum, min, max; J*_r
//                itself into the batch's rows when the caller wants the matrix.  No atomics: the order is fixed.
// Batches: RB = the replicates whose D fits JB_BATCH_BYTES (and the scan beside it as many again), at most JB_BATCH_MAX.
#pragma once

namespace {

constexpr size_t JB_BATCH_BYTES = 256u << 20;      // RB * n * 8 bytes <= 256 MB (twice: D and its scan)
constexpr int JB_BATCH_MAX = 64;
constexpr int JB_MAX_REP = 1024;

struct JbBuf {
    int n = 0; size_t cells = 0;
    DevBuf<long long> PM;                              // M's prefix, per slot
    DevBuf<long long> sum, mn, mx; DevBuf<int> sup;    // per fragment
    DevBuf<long long> D, P;                            // a batch: RB * n each (D: the terms, then J*_r per fragment)
};

void jb_free(JbBuf* b) { delete b; }

// Segmented inclusive sum with the run's head lane known: on return `v` of a run's last lane holds the run's sum.  Whole wave.
__device__ __forceinline__ long long jb_run_sum(long long v, int head)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long vu = __shfl_up(v, o, 64);
        if (lane - o >= head) v += vu;
    }
    return v;
}

// the lane at which the run of equal keys that holds this lane begins.  Whole wave.
__device__ __forceinline__ int jb_run_head(int key)
{
    const int lane = threadIdx.x & 63;
    const int kp = __shfl_up(key, 1, 64);
    int h = (lane == 0 || kp != key) ? lane : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int hu = __shfl_up(h, o, 64);
        if (lane >= o) h = max(h, hu);
    }
    return h;
}

__global__ __launch_bounds__(256) void k_jb_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt,
                                                long long nnz, const JnSub* __restrict__ sub, const JnFrag* __restrict__ fr, float nfpb, Par par,
                                                int quirk, unsigned long long seed, int r0, int rb, int n, long long* __restrict__ D,
                                                int* __restrict__ B)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {   // (wave-uniform bounds: the run sums need the whole wave)
        const long long k = k0 + lane;
        int ka = -1, kb = -1;
        unsigned ra = 0, cb = 0;
        double t = 0.0, ob = 0.0;
        bool has = false;
        if (k < nnz) {
            ra = (unsigned)row[k]; cb = (unsigned)col[k];
            const JnSub A = sub[ra], Bs = sub[cb];
            ka = A.slot; kb = Bs.slot;
            has = jn_contact_unit(A, Bs, fr, nfpb, par, quirk, t);
            if (has) ob = (double)__int_as_float(cnt[k]);
        }
        if (__ballot(has) == 0ull) continue;
        const int ha = jb_run_head(ka), hb = jb_run_head(kb);
        const int na = __shfl_down(ka, 1, 64), nb = __shfl_down(kb, 1, 64);   // (by every lane: a shuffle reads nothing from a lane that skips it)
        const bool ta = (lane == 63 || na != ka) && ka >= 0;
        const bool tb = (lane == 63 || nb != kb) && kb >= 0;
        const bool fwd = ka < kb;
        for (int r = 0; r < rb; r++) {
            long long c = 0;
            if (has) {
                SimStream st(ra, cb, 2u | ((unsigned)(r0 + r) << 8), seed);
                const long long q = to_q((double)sim_poisson(ob, st) * t);
                if (q == Q_BAD) jn_bad(B, ka, kb);
                else c = fwd ? q : -q;
            }
            const long long vr = jb_run_sum(c, ha), vc = jb_run_sum(-c, hb);
            long long* const Dr = D + (size_t)r * (size_t)n;
            if (ta && vr != 0) atomicAdd((unsigned long long*)&Dr[ka], (unsigned long long)vr);
            if (tb && vc != 0) atomicAdd((unsigned long long*)&Dr[kb], (unsigned long long)vc);
        }
    }
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
    // the batch: as many replicates as fit the bound, the same number whatever n_rep is (a replicate does not depend on it anyway)
    const int RB = (int)std::max<size_t>(1, std::min<size_t>(JB_BATCH_MAX, JB_BATCH_BYTES / (sizeof(long long) * (size_t)n)));
    const int rb_max = std::min(RB, (int)n_rep);
    if (!h->jb) h->jb = new JbBuf();
    JbBuf* X = h->jb;
    hipStream_t s = h->stream;
    const size_t cells = (size_t)rb_max * (size_t)n;
    size_t br = 0;
    CK(hipcub::DeviceScan::InclusiveSum(nullptr, br, (long long*)nullptr, (long long*)nullptr, (int)((size_t)RB * (size_t)n), s));
    if (const int rc = jn_reserve(h, br)) return rc;
    JnBuf* J = h->jn;
    CK(group_exact(X->n, (size_t)n, X->PM, n, X->sum, n, X->mn, n, X->mx, n, X->sup, n));
    CK(group_grow(X->cells, cells, X->D, cells, X->P, cells));
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
            STEP_CK(hipMemsetAsync(X->D, 0, sizeof(long long) * m, s));
            if (h->nnz > 0) {
                k_jb_nnz<<<stream_blocks(h->nnz), 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, J->sub, J->fr, h->nfpb, h->par, jn_quirk(h),
                                                               (unsigned long long)seed, r0, rb, n, X->D, J->B);
                STEP_CK(hipGetLastError());
            }
            size_t tb = J->L.tmp.count;
            STEP_CK(hipcub::DeviceScan::InclusiveSum(J->L.tmp.p, tb, X->D.p, X->P.p, (int)m, s));
            k_jb_fold<<<blocks_for(n, 256), 256, 0, s>>>(n, J->fr, X->PM, X->P, rb, r0 == 0 ? 1 : 0, (long long)threshold_q, X->sup, X->sum, X->mn,
                                                         X->mx, q_rep ? X->D.p : nullptr);
            STEP_CK(hipGetLastError());
            if (q_rep) {                                          // (the next batch clears D: the rows leave first)
                STEP_CK(hipMemcpyAsync(q_rep + (size_t)r0 * (size_t)n, X->D, sizeof(long long) * m, hipMemcpyDeviceToHost, s));
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
        // a junction that met an unrepresentable term (in the data or in a replicate) has no score: zeros, as at ends and in rings
        for (int f = 0; f < n; f++) {
            if (status[f] != GRAAL_JUNCTION_NONFINITE) continue;
            support[f] = 0; q_sum[f] = 0; q_min[f] = 0; q_max[f] = 0;
            if (q_rep) for (int r = 0; r < n_rep; r++) q_rep[(size_t)r * (size_t)n + f] = 0;
        }
    } while (false);
    return score_exit(h, "graal_junction_bootstrap", rc, nullptr, err);
}

} // extern "C"
