// simulate.h -- Hi-C contacts drawn from a layout under the engine's contact model (graal_simulate_contacts / graal_simulate_fetch).
// Included by graal_hip.hip after the C ABI (it uses Ctx, Geo, Stat, centre_kb, rippe, rippe_circ and model_math.h).
//
// Stands for the reference's simulate_data_2d (kernels3.cu:2331-2800, a dense Poisson draw per sub-pixel), whose host wrapper
// simulate_rippe_contacts cannot be called as written (cuda_lib_gl.py:1355 takes no arguments, simulation_loader.py:120 passes seven).
//
// Semantics: for every pair of sub-fragments a < b (both of active fragments) an independent count c ~ Poisson(lambda), lambda the
// expected value the full likelihood prices that sub-pixel with (ex_pair: rippe / rippe_circ of the float32 kb centres inside one contig,
// v_inter across contigs, times accu_a accu_b / n_frags_per_bins; the RF counts indexed exactly, not the trans-branch quirk; a negative
// value counts as 0).  The result is the COO list of the nonzero counts sorted by (row, col), row < col.
//
// Algorithm.  Outside the cis window (same contig, |centre_a - centre_b| < d_max) lambda is v_inter accu_a accu_b / nfpb.  So:
//  * window pairs are enumerated: the active sub-fragments are sorted by (contig, centre) once, a row's window is a contiguous range of
//    that order (two binary searches with the pricing's own float32 test), every pair in it with b > a is priced and drawn from its own
//    counter: inversion below lambda = 10, Hoermann's PTRS above;
//  * background pairs are not enumerated: a row's columns are cut into fixed chunks of SIM_CHUNK ids; inside a chunk, candidates come by
//    geometric skipping at p = 1 - e^-Lmax (Lmax = lambda with the largest RF count), a candidate b is kept with probability
//    (1 - e^-lambda_b) / p (thinning: window columns and inactive ones have lambda_b = 0 here) and gets a zero-truncated Poisson count;
//  * two passes over the same draws (count per row, exclusive scan, write), then every row is sorted by column in LDS (k_sim_place).
//
// RNG contract: Philox4x32-10 (Salmon et al., SC'11), key = (seed & 0xffffffff, seed >> 32).  A window pair (a, b) draws from counters
// (a, b, 0, n), background chunk k of row a from (a, k, 1, n), n = 0, 1, ...; each counter gives two uniforms in (0, 1), ((w1 w0) >> 12
// + 0.5) 2^-52 then ((w3 w2) >> 12 + 0.5) 2^-52.  Nothing depends on the grid: the list is a function of (layout, tables, parameters, seed).
// tests/sim_reference.py restates all of it in numpy.
#pragma once

namespace {   // (the engine's internals live in an anonymous namespace: Ctx's forward declarations are there)

constexpr int SIM_CHUNK = 4096;       // background chunk width (column ids)
constexpr int SIM_BLOCK = 256;
constexpr int SIM_KMAX = 256;         // inversion stops there (F has reached 1 long before for lambda < 10)
constexpr int SIM_TRIES = 64;         // rejection loops (PTRS accepts ~90 % per try)
constexpr double SIM_PTRS_MIN = 10.0;

struct SimRec { float centre; int label; int accu; int lbp; };   // label -1: inactive; lbp: contig length (bp) if circular, else -1

struct SimBuf {
    int S = 0;
    DevBuf<SimRec> rec;
    DevBuf<unsigned long long> key, key_s;
    DevBuf<int> val, order, inv, cnt;
    DevBuf<float> sc; DevBuf<int> sl;
    DevBuf<long long> off;
    DevBuf<void> tmp;
    DevBuf<int2> ent;                                   // grows (at least 1024 entries)
    DevBuf<int> orow, ocol, ocnt; long long out_cap = 0;
    DevBuf<unsigned> err;
    long long nnz = -1;
};

void sim_free(SimBuf* b) { delete b; }

// ---- Philox4x32-10 and the uniform stream
__device__ __forceinline__ uint4 philox4x32(uint4 c, unsigned k0, unsigned k1)
{
    for (int r = 0; r < 10; r++) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c.x, p1 = (unsigned long long)0xCD9E8D57u * c.z;
        c = make_uint4((unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0);
    }
    return c;
}

struct SimStream {
    unsigned c0, c1, c2, n, k0, k1;
    double u1; bool have;
    __device__ SimStream(unsigned a, unsigned b, unsigned tag, unsigned long long seed)
        : c0(a), c1(b), c2(tag), n(0), k0((unsigned)seed), k1((unsigned)(seed >> 32)), u1(0.0), have(false) {}
    __device__ __forceinline__ double next()
    {
        if (have) { have = false; return u1; }
        const uint4 w = philox4x32(make_uint4(c0, c1, c2, n++), k0, k1);
        const unsigned long long x0 = ((unsigned long long)w.y << 32) | w.x, x1 = ((unsigned long long)w.w << 32) | w.z;
        u1 = ((double)(x1 >> 12) + 0.5) * 0x1p-52;
        have = true;
        return ((double)(x0 >> 12) + 0.5) * 0x1p-52;
    }
};

// ln k! for k >= 0: the exact product below 17, Stirling's series (error < 1e-13) above
__device__ __forceinline__ double sim_lfact(long long k)
{
    if (k < 17) {
        double p = 1.0;
        for (int i = 2; i <= (int)k; i++) p = p * (double)i;
        return mm_ln_pos(p);
    }
    const double x = (double)(k + 1), x2 = x * x;
    return (x - 0.5) * mm_ln_pos(x) - x + 0.91893853320467274178 + 1.0 / (12.0 * x) - 1.0 / (360.0 * x * x2) + 1.0 / (1260.0 * x * x2 * x2);
}

__device__ int sim_poisson(double lam, SimStream& st)
{
    if (!(lam > 0.0)) return 0;
    if (lam < SIM_PTRS_MIN) {
        const double u = st.next();
        double p = mm_exp(-lam), F = p;
        int k = 0;
        while (u > F && k < SIM_KMAX) { k++; p = p * lam / (double)k; F = F + p; }
        return k;
    }
    const double slam = sqrt(lam), loglam = mm_ln_pos(lam);
    const double b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    for (int t = 0; t < SIM_TRIES; t++) {
        const double U = st.next() - 0.5, V = st.next();
        const double us = 0.5 - fabs(U);
        const double kf = floor((2.0 * a / us + b) * U + lam + 0.43);
        if (us >= 0.07 && V <= vr) return (int)kf;
        if (kf < 0.0 || (us < 0.013 && V > us)) continue;
        const long long k = (long long)kf;
        if (mm_ln_pos(V) + mm_ln_pos(invalpha) - mm_ln_pos(a / (us * us) + b) <= -lam + kf * loglam - sim_lfact(k)) return (int)k;
    }
    return (int)floor(lam + 0.5);
}

// zero-truncated Poisson
__device__ int sim_ztp(double lam, SimStream& st)
{
    if (lam < SIM_PTRS_MIN) {
        const double u = st.next();
        const double p0 = mm_exp(-lam);
        const double t = p0 + u * (1.0 - p0);
        double p = p0, F = p0;
        int k = 0;
        while (t > F && k < SIM_KMAX) { k++; p = p * lam / (double)k; F = F + p; }
        return k > 0 ? k : 1;
    }
    for (int t = 0; t < SIM_TRIES; t++) {
        const int k = sim_poisson(lam, st);
        if (k > 0) return k;
    }
    return 1;
}

// expected value of a window pair (ex_pair's cis branch) and of a background pair (its trans value)
__device__ __forceinline__ float sim_norm(int aa, int ab, float nfpb) { return (float)(aa * ab) / nfpb; }
__device__ __forceinline__ double sim_lam_window(const SimRec& A, const SimRec& B, float nfpb, const Par& p)
{
    const float norm = sim_norm(A.accu, B.accu, nfpb);
    const float s = fabsf(B.centre - A.centre);
    const float v = (A.lbp >= 0 ? rippe_circ(s, (float)A.lbp / 1000.0f, p) : rippe(s, p)) * norm;
    return v > 0.0f ? (double)v : 0.0;
}

// ---- preparation: per sub-fragment record and sort key (contig, centre); inactive sub-fragments sort last
__global__ __launch_bounds__(256) void k_sim_prep(int n, const Geo* __restrict__ geo, const Stat* __restrict__ stat, const int* __restrict__ sub_ids,
                                                 const int* __restrict__ lcontbp, SimRec* __restrict__ rec, unsigned long long* __restrict__ key,
                                                 int* __restrict__ val)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const Stat st = stat[f];
    const Geo g = geo[f];
    const bool fwd = g.flags & 1, active = geo_active(g.flags), circ = (g.flags >> 1) & 1;
    int4 ids = make_int4(f, 0, 0, 1);
    if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[f];
    for (int slot = 0; slot < st.n; slot++) {
        const int id = sel3(ids.x, ids.y, ids.z, slot);
        SimRec r;
        r.centre = centre_kb(g.start_bp, fwd, st, slot);
        r.label = active ? g.id_c : -1;
        r.accu = stat_accu(st, slot);
        r.lbp = circ ? lcontbp[f] : -1;
        rec[id] = r;
        unsigned cb = __float_as_uint(r.centre);
        cb = (cb & 0x80000000u) ? ~cb : (cb | 0x80000000u);           // order-preserving bits of a float
        key[id] = active ? (((unsigned long long)(unsigned)g.id_c << 32) | cb) : ~0ull;
        val[id] = id;
    }
}

__global__ void k_sim_sorted(int S, const int* __restrict__ order, const SimRec* __restrict__ rec, int* __restrict__ inv, float* __restrict__ sc,
                             int* __restrict__ sl)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= S) return;
    const int id = order[j];
    inv[id] = j;
    sc[j] = rec[id].centre;
    sl[j] = rec[id].label;
}

// One row per block.  WRITE = false: cnt[a] = nonzero entries of row a.  WRITE = true: the same draws, entries (col, count) appended to
// row a's segment ent[off[a] .. off[a + 1]) in any order (placed by k_sim_place).
template <bool WRITE>
__global__ __launch_bounds__(SIM_BLOCK) void k_sim_rows(int S, const SimRec* __restrict__ rec, const int* __restrict__ order,
                                                         const int* __restrict__ inv, const float* __restrict__ sc, const int* __restrict__ sl,
                                                         Par par, float nfpb, int amax, unsigned long long seed, int* __restrict__ cnt,
                                                         const long long* __restrict__ off, int2* __restrict__ ent, unsigned* __restrict__ err)
{
    __shared__ int s_n;
    __shared__ int s_lohi[2];
    const int a = blockIdx.x;
    const SimRec A = rec[a];
    if (threadIdx.x == 0) s_n = 0;
    const bool active = A.label >= 0;
    if (active && threadIdx.x < 2) {
        // window of a in the sorted order: [lo, hi) = the entries of a's contig with |centre - centre_a| < d_max (contiguous: the
        // float32 difference is monotone in the sorted centre)
        const int ja = inv[a];
        int lo, hi;
        if (threadIdx.x == 0) {
            lo = 0; hi = ja;           // first j in [0, ja] inside
            while (lo < hi) { const int m = (lo + hi) >> 1; if (sl[m] == A.label && fabsf(sc[m] - A.centre) < par.d_max) hi = m; else lo = m + 1; }
            s_lohi[0] = lo;
        }
        else {
            lo = ja + 1; hi = S;       // first j in (ja, S] outside
            while (lo < hi) { const int m = (lo + hi) >> 1; if (!(sl[m] == A.label && fabsf(sc[m] - A.centre) < par.d_max)) hi = m; else lo = m + 1; }
            s_lohi[1] = lo;
        }
    }
    __syncthreads();
    if (!active) { if (!WRITE && threadIdx.x == 0) cnt[a] = 0; return; }
    const long long base = WRITE ? off[a] : 0;
    const int cap = WRITE ? (int)(off[a + 1] - base) : 0;
    int mine = 0;
    auto emit = [&](int col, int c) {
        if (WRITE) {
            const int slot = atomicAdd(&s_n, 1);
            if (slot < cap) ent[base + slot] = make_int2(col, c);
            else atomicOr(err, 1u);
        }
        else mine++;
    };
    // window pairs
    for (int j = s_lohi[0] + (int)threadIdx.x; j < s_lohi[1]; j += SIM_BLOCK) {
        const int b = order[j];
        if (b <= a) continue;
        const double lam = sim_lam_window(A, rec[b], nfpb, par);
        if (!(lam > 0.0)) continue;
        SimStream st((unsigned)a, (unsigned)b, 0u, seed);
        const int c = sim_poisson(lam, st);
        if (c > 0) emit(b, c);
    }
    // background chunks
    const float lmax_f = par.v_inter * sim_norm(A.accu, amax, nfpb);
    if (lmax_f > 0.0f) {
        const double lmax = (double)lmax_f, pm = 1.0 - mm_exp(-lmax);
        const int k0 = (a + 1) / SIM_CHUNK, k1 = (S - 1) / SIM_CHUNK;
        for (int k = k0 + (int)threadIdx.x; k <= k1; k += SIM_BLOCK) {
            const int c_begin = max(a + 1, k * SIM_CHUNK), c_end = min(S, (k + 1) * SIM_CHUNK);
            SimStream st((unsigned)a, (unsigned)k, 1u, seed);
            int j = c_begin - 1;
            while (true) {
                const double g = -mm_ln_pos(st.next()) / lmax;      // failures before the next candidate
                if (!(g < (double)(c_end - j - 1))) break;
                j = j + 1 + (int)floor(g);
                const SimRec B = rec[j];
                if (B.label < 0) continue;
                if (B.label == A.label && fabsf(B.centre - A.centre) < par.d_max) continue;   // a window pair
                const float lb = par.v_inter * sim_norm(A.accu, B.accu, nfpb);
                const double v = st.next();
                const double qb = 1.0 - mm_exp(-(double)lb);
                if (v * pm < qb) emit(j, sim_ztp((double)lb, st));
            }
        }
    }
    if (!WRITE) {
        for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
        if ((threadIdx.x & 63) == 0) atomicAdd(&s_n, mine);
        __syncthreads();
        if (threadIdx.x == 0) cnt[a] = s_n;
    }
    else {
        __syncthreads();
        if (threadIdx.x == 0 && s_n != cap) atomicOr(err, 2u);
    }
}

__global__ void k_sim_off_tail(int S, const int* __restrict__ cnt, long long* __restrict__ off)
{
    off[S] = off[S - 1] + (long long)cnt[S - 1];
}

// Rows come out sorted by column without a global sort (columns of a row are distinct).  A row of at most SIM_BLOCK entries (C5: ~135
// on average) places each entry at its rank in one pass over the row in LDS.  A row of at most SIM_SORT entries is sorted in LDS by a
// bitonic network on (col << 32 | count) keys: O(n log^2 n) per row.  A longer row places every entry at its rank, scanning the row in
// LDS tiles: O(n^2 / SIM_BLOCK) per thread, for the rare very dense row only.
constexpr int SIM_SORT = 4096;
__global__ __launch_bounds__(SIM_BLOCK) void k_sim_place(const long long* __restrict__ off, const int2* __restrict__ ent, int* __restrict__ orow,
                                                          int* __restrict__ ocol, int* __restrict__ ocnt, unsigned* __restrict__ err)
{
    __shared__ unsigned long long key[SIM_SORT];
    const int a = blockIdx.x;
    const long long base = off[a];
    const int n = (int)(off[a + 1] - base);
    if (n == 0) return;
    if (n <= SIM_BLOCK) {                             // one entry per thread: its rank in one pass over the row in LDS
        int* col = reinterpret_cast<int*>(key);
        const int2 me = (int)threadIdx.x < n ? ent[base + threadIdx.x] : make_int2(0x7fffffff, 0);
        col[threadIdx.x] = me.x;
        __syncthreads();
        if ((int)threadIdx.x < n) {
            int rank = 0;
            for (int i = 0; i < n; i++) rank += col[i] < me.x ? 1 : 0;
            orow[base + rank] = a; ocol[base + rank] = me.x; ocnt[base + rank] = me.y;
        }
        return;
    }
    if (n <= SIM_SORT) {
        int P = 1;
        while (P < n) P <<= 1;
        for (int i = threadIdx.x; i < P; i += SIM_BLOCK) {
            if (i < n) { const int2 e = ent[base + i]; key[i] = ((unsigned long long)(unsigned)e.x << 32) | (unsigned)e.y; }
            else key[i] = ~0ull;
        }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = threadIdx.x; i < P; i += SIM_BLOCK) {
                    const int l = i ^ j;
                    if (l > i) {
                        const unsigned long long x = key[i], y = key[l];
                        if (((i & k) == 0) == (x > y)) { key[i] = y; key[l] = x; }
                    }
                }
                __syncthreads();
            }
        for (int i = threadIdx.x; i < n; i += SIM_BLOCK) {
            const unsigned long long x = key[i];
            orow[base + i] = a; ocol[base + i] = (int)(x >> 32); ocnt[base + i] = (int)(unsigned)x;
        }
        return;
    }
    int* tile = reinterpret_cast<int*>(key);          // (2 * SIM_SORT column ids per tile)
    for (int e0 = 0; e0 < n; e0 += SIM_BLOCK) {
        const int e = e0 + (int)threadIdx.x;
        const int2 me = e < n ? ent[base + e] : make_int2(0x7fffffff, 0);
        int rank = 0;
        for (int t0 = 0; t0 < n; t0 += 2 * SIM_SORT) {
            const int m = min(2 * SIM_SORT, n - t0);
            __syncthreads();
            for (int i = threadIdx.x; i < m; i += SIM_BLOCK) tile[i] = ent[base + t0 + i].x;
            __syncthreads();
            for (int i = 0; i < m; i++) rank += tile[i] < me.x ? 1 : 0;
        }
        if (e < n) {
            if (rank < n) { orow[base + rank] = a; ocol[base + rank] = me.x; ocnt[base + rank] = me.y; }
            else atomicOr(err, 4u);
        }
    }
}

} // namespace

extern "C" {

int graal_simulate_contacts(graal_ctx* h, uint64_t seed, int64_t* nnz_out)
{
    if (!h || !nnz_out) return GRAAL_E_ARG;
    *nnz_out = 0;
    if (!(h->have_sub && h->have_par && h->have_frags)) return fail(h, GRAAL_E_STATE, "upload sub-fragments, parameters and fragments first");
    if (h->has_rep) return fail(h, GRAAL_E_UNSUPPORTED, "graal_simulate_contacts: bins with several copies (graal_upload_repeats) are not supported");
    if (!h->order_valid) { int32_t m = 0; const int rc = graal_relabel_contigs(h, &m); if (rc) return rc; }
    CK(hipSetDevice(h->device));
    CK(hipStreamSynchronize(h->fstream));
    const int S = h->n_sub_total, n = h->n;
    if (S < 2) { if (h->sim) h->sim->nnz = 0; else { h->sim = new SimBuf(); h->sim->nnz = 0; } return GRAAL_OK; }
    if (!h->sim) h->sim = new SimBuf();
    SimBuf* B = h->sim;
    B->nnz = -1;
    hipStream_t s = h->stream;
    if (B->S != S) {
        size_t b1 = 0, b2 = 0;
        CK(hipcub::DeviceRadixSort::SortPairs(nullptr, b1, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int*)nullptr, (int*)nullptr,
                                              S, 0, 64, s));
        CK(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, (int*)nullptr, (long long*)nullptr, S, s));
        CK(group_realloc(B->S, S, B->rec, S, B->key, S, B->key_s, S, B->val, S, B->order, S, B->inv, S, B->cnt, S, B->sc, S, B->sl, S, B->off, S + 1,
                         B->err, 1, B->tmp, std::max(b1, b2)));
    }
    int amax = 1;
    for (int b = 0; b < h->n_bins; b++)
        for (int t = 0; t < h->h_nsub[b]; t++) amax = std::max(amax, h->h_accu[3 * (size_t)b + t]);
    // (rows without a sub-fragment record -- none: every sub-fragment id belongs to one bin slot, graal_upload_subfrags checks it)
    k_sim_prep<<<blocks_for(n, 256), 256, 0, s>>>(n, h->geo, h->stat_frag, h->d_sub_ids, h->soa[h->cur].p[F_LCONTBP], B->rec, B->key, B->val);
    CK(hipGetLastError());
    size_t tb = B->tmp.count;
    CK(hipcub::DeviceRadixSort::SortPairs(B->tmp.p, tb, B->key.p, B->key_s.p, B->val.p, B->order.p, S, 0, 64, s));
    k_sim_sorted<<<blocks_for(S, 256), 256, 0, s>>>(S, B->order, B->rec, B->inv, B->sc, B->sl);
    CK(hipGetLastError());
    CK(hipMemsetAsync(B->err, 0, sizeof(unsigned), s));
    k_sim_rows<false><<<S, SIM_BLOCK, 0, s>>>(S, B->rec, B->order, B->inv, B->sc, B->sl, h->par, h->nfpb, amax, (unsigned long long)seed, B->cnt,
                                               nullptr, nullptr, B->err);
    CK(hipGetLastError());
    tb = B->tmp.count;
    CK(hipcub::DeviceScan::ExclusiveSum(B->tmp.p, tb, B->cnt.p, B->off.p, S, s));
    k_sim_off_tail<<<1, 1, 0, s>>>(S, B->cnt, B->off);
    CK(hipGetLastError());
    long long nnz = 0;
    CK(hipMemcpyAsync(&nnz, B->off + S, sizeof(long long), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    const size_t out = (size_t)std::max<long long>(nnz, 1024);
    if ((size_t)nnz > B->ent.count) CK(B->ent.alloc(out));
    if (nnz > B->out_cap) CK(group_realloc(B->out_cap, out, B->orow, out, B->ocol, out, B->ocnt, out));
    if (nnz > 0) {
        k_sim_rows<true><<<S, SIM_BLOCK, 0, s>>>(S, B->rec, B->order, B->inv, B->sc, B->sl, h->par, h->nfpb, amax, (unsigned long long)seed,
                                                  B->cnt, B->off, B->ent, B->err);
        CK(hipGetLastError());
        k_sim_place<<<S, SIM_BLOCK, 0, s>>>(B->off, B->ent, B->orow, B->ocol, B->ocnt, B->err);
        CK(hipGetLastError());
    }
    unsigned err = 0;
    CK(hipMemcpyAsync(&err, B->err, sizeof(unsigned), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (err) {
        char m[128];
        snprintf(m, sizeof m, "graal_simulate_contacts: the write pass disagreed with the count pass (flags %u)", err);
        h->err = m;
        return GRAAL_E_STATE;
    }
    B->nnz = nnz;
    *nnz_out = nnz;
    return GRAAL_OK;
}

int graal_simulate_fetch(graal_ctx* h, int32_t* row, int32_t* col, int32_t* count, int64_t cap)
{
    if (!h || !row || !col || !count) return GRAAL_E_ARG;
    if (!h->sim || h->sim->nnz < 0) return fail(h, GRAAL_E_STATE, "graal_simulate_fetch: call graal_simulate_contacts first");
    const long long nnz = h->sim->nnz;
    if (cap < nnz) return fail(h, GRAAL_E_ARG, "graal_simulate_fetch: cap is smaller than the list");
    if (nnz == 0) return GRAAL_OK;
    CK(hipSetDevice(h->device));
    CK(hipMemcpyAsync(row, h->sim->orow, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, h->stream));
    CK(hipMemcpyAsync(col, h->sim->ocol, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, h->stream));
    CK(hipMemcpyAsync(count, h->sim->ocnt, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost, h->stream));
    CK(hipStreamSynchronize(h->stream));
    return GRAAL_OK;
}

} // extern "C"
