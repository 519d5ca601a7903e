// map_windows.h -- windows of the genome-order maps at any bin size, many per call (graal_map_windows / graal_map_windows_fetch;
// semantics in include/graal_hip.h).  Included by graal_hip.hip after maps.h (it uses map_window.h's geometry, score_common.h,
// layout_slots.h's LayoutSlots, junctions.h's k_jn_prep, JnFrag and JnSub, and maps.h's k_mp_slots, k_mp_rank, mp_pair_q, mp_pixel and
// MP_O_SCALE).
//
// A window is an origin (u0, v0) in ranks of maps.h's order and a shared (px_rows, px_cols, bin); pixel (p, q) sums the bin-1 matrix over
// its row ranks x its column ranks (map_window.h), every ordered pair a != b.  The cost follows what the windows hold: the contact list is
// streamed once per call whatever the number of windows, and only the rank pairs inside the windows are priced.
//
// Kernels, all on the engine's stream:
//   slots_count / k_jn_prep / k_mp_slots / scan / k_mp_rank at bin 1 -- maps.h's own: slots, ranks, rank_of_sub, the RF count and its square
//                per rank; two more exclusive scans (int64, S + 1 entries) turn those into prefix sums over ranks, so that the sums over a
//                pixel's rows, its columns and their overlap are two subtractions each;
//   k_mw_rec   -- a 32-byte record per RANK: centre as the pricing has it, RF count, the contig's key (its last slot), the slot, the
//                fragment's bp interval (k_mp_cis's reach test), the ring's length and flag;
//   k_mw_cover -- a bitmap over ranks: set where some window's rows or columns reach;
//   k_mw_obs   -- streams the contact list, 64 consecutive contacts per wave.  Every block copies the bitmap into LDS first (S bits; it
//                stays in global memory beyond 64 KB of them) and a contact whose two ranks are not both covered is dropped there.  A
//                survivor finds its windows by a binary search in the windows sorted by row origin -- those with u0 in (a - rows, a] are
//                consecutive -- tests each one's columns and adds count * 2^24 (rounded once, k_mp_obs's value) with one int64 atomic per
//                window and direction;
//   k_mw_exp_t -- bin <= 8: one thread per pixel, its bin x bin rank pairs summed in a register;
//   k_mw_exp_w -- bin > 8: a block owns one pixel row of a window and a run of column pixels (512 ranks' worth).  The run's column records
//                and the row's records are staged in LDS once; each wave then takes pixels of the run, its lanes the pixel's rank pairs;
//                the sum is reduced inside the wave and written once.  A pixel whose rows and columns share no contig, or lie in one
//                linear contig beyond its reach, is known from four records and costs no pair.  A pixel wider than 512 ranks is a
//                block's own: the column records pass through LDS 512 at a time, the threads hold the row ranks, and tiles of another
//                contig or beyond the reach of a linear one are skipped from their first and last record;
//   k_mw_out   -- per pixel: the background from the prefix sums, then maps.h's mp_pixel (the arithmetic of k_mp_out).
// No atomics on the expected side: every pixel has one owner, and int64 sums do not depend on the order of their terms.
#pragma once

namespace {

constexpr int MW_THREAD_BIN = 8;     // up to this bin a thread owns a pixel, beyond it a wave or a block
constexpr int MW_TILE = 512;         // ranks staged in LDS per side (32 bytes each)
constexpr size_t MW_LDS_BITMAP_BYTES = 65536;

struct MwRec { float centre; int accu; int key; int slot; int start_bp; int end_bp; float s_tot; int circ; };   // per rank, 32 bytes

struct MwBuf {
    int n = 0, S = 0;                         // the layout buffers' sizes
    LayoutSlots L;                            // (its tmp also serves the scans of nsub and of the RF counts)
    DevBuf<int> nsub, rank0, lbp, rank_of;
    DevBuf<JnFrag> fr;
    DevBuf<JnSub> sub;
    DevBuf<MwRec> rec;
    DevBuf<long long> A, A2;                  // per rank: the RF count and its square (S + 1 entries, the last 0)
    DevBuf<long long> PA, PA2;                // their exclusive prefix sums (S + 1 entries)
    DevBuf<unsigned> cover;                   // the bitmap over ranks
    DevBuf<unsigned long long> nbad;
    DevBuf<int> win;                          // [5][n_win]: u0, v0 in the caller's order; u0, v0, image index sorted by u0 (it only grows)
    size_t px_cap = 0;                        // pixels the image buffers hold (they only grow)
    DevBuf<long long> O, E;
    DevBuf<unsigned char> badf;
    DevBuf<float> obs, exp, res;
    int n_win = 0, pr = 0, pc = 0;
    bool valid = false;                       // the images are those of a finished call
};

void mw_free(MwBuf* b) { delete b; }

// per slot: the record of each of its ranks (k_mp_rank has checked that the ranks add up)
__global__ void k_mw_rec(int n, int S, const JnFrag* __restrict__ fr, const int* __restrict__ rank0, const int* __restrict__ lbp_of,
                         MwRec* __restrict__ rec)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const JnFrag r = fr[i];
    const int r0 = rank0[i];
    if (r0 < 0 || r.n < 0 || r.n > 3 || r0 + r.n > S) return;
    MwRec u;
    u.key = min(r.last, n - 1); u.slot = i; u.start_bp = r.start_bp; u.end_bp = r.start_bp + r.len_bp;
    u.s_tot = (float)lbp_of[i] / 1000.0f; u.circ = (r.flags & 2) ? 1 : 0;
    for (int k = 0; k < r.n; k++) {
        u.centre = sel3(r.c0, r.c1, r.c2, k);
        u.accu = sel3(r.a0, r.a1, r.a2, k);
        rec[r0 + ((r.flags & 1) ? k : r.n - 1 - k)] = u;
    }
}

// one thread per window and side: the bits of the ranks it reaches
__global__ void k_mw_cover(int n_win, const int* __restrict__ u0, const int* __restrict__ v0, int pr, int pc, int bin, int S,
                           unsigned* __restrict__ cover)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * n_win) return;
    const MwRange r = (t & 1) ? mw_span_ranks(v0[t >> 1], 0, pc, bin, S) : mw_span_ranks(u0[t >> 1], 0, pr, bin, S);
    if (r.hi <= r.lo) return;
    const int w0 = r.lo >> 5, w1 = (r.hi - 1) >> 5;
    for (int w = w0; w <= w1; w++) {
        unsigned m = 0xffffffffu;
        if (w == w0) m &= 0xffffffffu << (r.lo & 31);
        if (w == w1) m &= 0xffffffffu >> (31 - ((r.hi - 1) & 31));
        atomicOr(&cover[w], m);
    }
}

// the contact's value into every window whose rows hold rank a and whose columns hold rank b
__device__ __forceinline__ void mw_scatter(int a, int b, long long v, int n_win, const int* __restrict__ su0, const int* __restrict__ sv0,
                                           const int* __restrict__ simg, int pr, int pc, int bin, long long* __restrict__ O)
{
    const long long first = (long long)a - (long long)pr * (long long)bin;   // windows with u0 in (first, a]
    int lo = 0, hi = n_win;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)su0[mid] <= first) lo = mid + 1; else hi = mid;
    }
    for (int w = lo; w < n_win; w++) {
        const int u0 = su0[w];
        if (u0 > a) break;
        const int q = mw_pixel_of(b, sv0[w], pc, bin);
        if (q < 0) continue;
        const int p = mw_pixel_of(a, u0, pr, bin);
        if (p < 0) continue;
        atomicAdd((unsigned long long*)&O[((long long)simg[w] * pr + p) * pc + q], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void k_mw_obs(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt, long long nnz,
                                                const int* __restrict__ rank_of, const unsigned* __restrict__ cover, int words, int in_lds,
                                                int n_win, const int* __restrict__ su0, const int* __restrict__ sv0,
                                                const int* __restrict__ simg, int pr, int pc, int bin, long long* __restrict__ O)
{
    extern __shared__ unsigned s_cover[];
    if (in_lds) {
        for (int t = threadIdx.x; t < words; t += blockDim.x) s_cover[t] = cover[t];
        __syncthreads();
    }
    const unsigned* const bm = in_lds ? s_cover : cover;
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {
        const long long k = k0 + lane;
        if (k >= nnz) continue;
        const int r = row[k], c = col[k];
        if (r == c) continue;
        const int a = rank_of[r], b = rank_of[c];
        if (a < 0 || b < 0) continue;
        if (!((bm[a >> 5] >> (a & 31)) & (bm[b >> 5] >> (b & 31)) & 1u)) continue;
        const long long v = __double2ll_rn((double)__int_as_float(cnt[k]) * MP_O_SCALE);
        if (v == 0) continue;
        mw_scatter(a, b, v, n_win, su0, sv0, simg, pr, pc, bin, O);
        mw_scatter(b, a, v, n_win, su0, sv0, simg, pr, pc, bin, O);
    }
}

// What the pair of ranks (ra, rb) adds to a pixel beyond the background: mp_pair_q for two ranks of one contig (inside the reach of a linear
// one: k_mp_cis's test on the two fragments), else 0.  Q_BAD: a term that is not finite or does not fit.
__device__ __forceinline__ long long mw_term(const MwRec& x, const MwRec& y, int ra, int rb, float nfpb, const Par& par, int reach_bp)
{
    if (x.key != y.key || ra == rb) return 0;
    const bool x_first = x.slot <= y.slot;
    const MwRec& lo = x_first ? x : y;
    const MwRec& hi = x_first ? y : x;
    const bool circ = lo.circ != 0;
    if (!circ && lo.slot != hi.slot && hi.start_bp - lo.end_bp > reach_bp) return 0;   // beyond the window: cis = trans exactly
    return mp_pair_q(lo.centre, hi.centre, lo.accu, hi.accu, circ, lo.s_tot, nfpb, par);
}

__global__ __launch_bounds__(256) void k_mw_exp_t(int n_win, const int* __restrict__ u0, const int* __restrict__ v0, int pr, int pc, int bin, int S,
                                                  const MwRec* __restrict__ rec, float nfpb, Par par, int reach_bp, long long* __restrict__ E,
                                                  unsigned char* __restrict__ badf)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)pr * pc;
    if (idx >= (long long)n_win * per) return;
    const int w = (int)(idx / per), rest = (int)(idx - (long long)w * per), p = rest / pc, q = rest - p * pc;
    const MwRange R = mw_pixel_ranks(u0[w], p, bin, S), C = mw_pixel_ranks(v0[w], q, bin, S);
    long long acc = 0;
    bool bad = false;
    for (int a = R.lo; a < R.hi; a++) {
        const MwRec x = rec[a];
        for (int b = C.lo; b < C.hi; b++) {
            const MwRec y = rec[b];
            const long long t = mw_term(x, y, a, b, nfpb, par, reach_bp);
            if (t == Q_BAD) bad = true; else acc += t;
        }
    }
    E[idx] = acc;
    badf[idx] = bad ? 1 : 0;
}

__device__ __forceinline__ long long mw_wave_sum(long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void k_mw_exp_w(int n_win, const int* __restrict__ u0, const int* __restrict__ v0, int pr, int pc, int bin, int S,
                                                  int run, int runs, const MwRec* __restrict__ rec, float nfpb, Par par, int reach_bp,
                                                  long long* __restrict__ E, unsigned char* __restrict__ badf)
{
    __shared__ MwRec s_row[MW_TILE];
    __shared__ MwRec s_col[MW_TILE];
    __shared__ long long s_sum[4];
    __shared__ int s_bad[4];
    const int tid = threadIdx.x, lane = tid & 63, wib = tid >> 6;
    const int g = blockIdx.x % runs, wp = blockIdx.x / runs, p = wp % pr, w = wp / pr;   // (the grid is n_win * pr * runs blocks)
    const int q0 = g * run, nq = min(run, pc - q0);
    const long long base = ((long long)w * pr + p) * pc + q0;
    const MwRange R = mw_pixel_ranks(u0[w], p, bin, S);
    if (bin <= MW_TILE) {
        const MwRange Cs = mw_span_ranks(v0[w], q0, nq, bin, S);
        const int nr = R.hi - R.lo;
        for (int t = tid; t < nr; t += 256) s_row[t] = rec[R.lo + t];
        for (int t = tid; t < Cs.hi - Cs.lo; t += 256) s_col[t] = rec[Cs.lo + t];
        __syncthreads();
        for (int qq = wib; qq < nq; qq += 4) {                // (wave-uniform)
            const MwRange C = mw_pixel_ranks(v0[w], q0 + qq, bin, S);
            const int nc = C.hi - C.lo, c_off = C.lo - Cs.lo;
            long long acc = 0;
            int bad = 0;
            bool none = nr < 1 || nc < 1;                     // (wave-uniform) no pair of the pixel has a term
            if (!none) {
                const MwRec &r0 = s_row[0], &r1 = s_row[nr - 1], &c0 = s_col[c_off], &c1 = s_col[c_off + nc - 1];
                none = r1.key < c0.key || c1.key < r0.key;    // (keys grow with the rank) rows and columns share no contig
                if (!none && r0.key == r1.key && c0.key == c1.key && !r0.circ)   // one linear contig (start_bp grows along it):
                    none = (c0.slot > r1.slot && c0.start_bp - r1.end_bp > reach_bp) || (r0.slot > c1.slot && r0.start_bp - c1.end_bp > reach_bp);
            }                                                 // every pair beyond the reach, as mw_term would find one by one
            for (int t = lane; t < (none ? 0 : nr * nc); t += 64) {
                const int a = t / nc, b = t - a * nc;
                const long long v = mw_term(s_row[a], s_col[c_off + b], R.lo + a, C.lo + b, nfpb, par, reach_bp);
                if (v == Q_BAD) bad = 1; else acc += v;
            }
            acc = mw_wave_sum(acc);                           // (every lane is back here: the loop above is the only divergence)
            const bool any_bad = __ballot(bad != 0) != 0ull;
            if (lane == 0) { E[base + qq] = acc; badf[base + qq] = any_bad ? 1 : 0; }
        }
        return;
    }
    // a pixel wider than a tile: run == 1, the block's one pixel
    const MwRange C = mw_pixel_ranks(v0[w], q0, bin, S);
    long long acc = 0;
    int bad = 0;
    for (int c0 = C.lo; c0 < C.hi; c0 += MW_TILE) {           // (block-uniform)
        const int cnt = min(MW_TILE, C.hi - c0);
        __syncthreads();                                      // (the tile before has been read)
        for (int t = tid; t < cnt; t += 256) s_col[t] = rec[c0 + t];
        __syncthreads();
        const MwRec first = s_col[0], last = s_col[cnt - 1];
        for (int a = R.lo + tid; a < R.hi; a += 256) {
            const MwRec x = rec[a];
            if (first.key > x.key || last.key < x.key) continue;                     // (keys grow with the rank) another contig's tile
            if (!x.circ) {                                                           // (start_bp grows along a contig)
                if (first.key == x.key && first.slot > x.slot && first.start_bp - x.end_bp > reach_bp) continue;
                if (last.key == x.key && last.slot < x.slot && x.start_bp - last.end_bp > reach_bp) continue;
            }
            for (int b = 0; b < cnt; b++) {
                const long long v = mw_term(x, s_col[b], a, c0 + b, nfpb, par, reach_bp);
                if (v == Q_BAD) bad = 1; else acc += v;
            }
        }
    }
    acc = mw_wave_sum(acc);
    const bool any_bad = __ballot(bad != 0) != 0ull;
    if (lane == 0) { s_sum[wib] = acc; s_bad[wib] = any_bad ? 1 : 0; }
    __syncthreads();
    if (tid == 0) {
        E[base] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
        badf[base] = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void k_mw_out(int n_win, const int* __restrict__ u0, const int* __restrict__ v0, int pr, int pc, int bin, int S,
                                                const long long* __restrict__ O, const long long* __restrict__ E,
                                                const unsigned char* __restrict__ badf, const long long* __restrict__ PA,
                                                const long long* __restrict__ PA2, double v_over_nfpb, float* __restrict__ obs,
                                                float* __restrict__ exp_, float* __restrict__ res, unsigned long long* __restrict__ nbad)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)pr * pc;
    if (idx >= (long long)n_win * per) return;
    const int w = (int)(idx / per), rest = (int)(idx - (long long)w * per), p = rest / pc, q = rest - p * pc;
    const MwRange R = mw_pixel_ranks(u0[w], p, bin, S), C = mw_pixel_ranks(v0[w], q, bin, S);
    float of = 0.0f, ef = 0.0f, rf = 0.0f;
    if (R.hi > R.lo && C.hi > C.lo) {         // (a pixel outside the genome is 0 everywhere and never bad)
        const MwRange I = mw_overlap(R, C);
        const long long ar = PA[R.hi] - PA[R.lo], ac = PA[C.hi] - PA[C.lo], a2 = PA2[I.hi] - PA2[I.lo];
        // sum of accu_a accu_b over the pixel's ordered pairs a != b
        const double pairs = (ar < (1ll << 31) && ac < (1ll << 31)) ? (double)(ar * ac - a2) : (double)ar * (double)ac - (double)a2;
        if (mp_pixel(O[idx], E[idx], 1.0, pairs, v_over_nfpb, badf[idx] != 0, of, ef, rf)) atomicAdd(nbad, 1ull);
    }
    obs[idx] = of;
    exp_[idx] = ef;
    res[idx] = rf;
}

} // namespace

extern "C" {

int graal_map_windows(graal_ctx* h, int32_t n_win, const int32_t* origin, int32_t px_rows, int32_t px_cols, int32_t bin, int64_t* bad_pixels_out)
{
    if (!h) return GRAAL_E_ARG;
    if (n_win < 1 || !origin) return fail(h, GRAAL_E_ARG, "graal_map_windows: at least one window and its origin are needed");
    if (px_rows < 1 || px_rows > GRAAL_MAPS_MAX_PX || px_cols < 1 || px_cols > GRAAL_MAPS_MAX_PX)
        return fail(h, GRAAL_E_ARG, "graal_map_windows: px_rows and px_cols must lie in 1 .. 4096");
    if (bin < 1) return fail(h, GRAAL_E_ARG, "graal_map_windows: bin must be at least 1");
    const long long budget = (long long)GRAAL_MAPS_MAX_PX * GRAAL_MAPS_MAX_PX;
    if ((long long)n_win * px_rows * px_cols > budget)
        return fail(h, GRAAL_E_ARG, "graal_map_windows: the windows hold more than 4096 x 4096 pixels in all");
    if (const int rc = score_entry(h, "graal_map_windows")) return rc;
    const int n = h->n, S = h->n_sub_total;
    if (!h->mw) h->mw = new MwBuf();
    MwBuf* M = h->mw;
    M->valid = false;
    if (bad_pixels_out) *bad_pixels_out = 0;
    hipStream_t s = h->stream;
    const size_t px = (size_t)n_win * (size_t)px_rows * (size_t)px_cols;
    CK(group_grow(M->px_cap, px, M->O, px, M->E, px, M->badf, px, M->obs, px, M->exp, px, M->res, px));
    if (n < 1 || S < 1) {                     // no genome: every pixel lies outside it
        CK(hipMemsetAsync(M->obs, 0, sizeof(float) * px, s));
        CK(hipMemsetAsync(M->exp, 0, sizeof(float) * px, s));
        CK(hipMemsetAsync(M->res, 0, sizeof(float) * px, s));
        CK(hipStreamSynchronize(s));
        M->n_win = n_win; M->pr = px_rows; M->pc = px_cols; M->valid = true;
        return GRAAL_OK;
    }
    const int words = (S + 31) / 32;
    if (M->n != n || M->S != S) {
        size_t b2 = 0, b3 = 0;
        CK(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, (int*)nullptr, (int*)nullptr, n, s));
        CK(hipcub::DeviceScan::ExclusiveSum(nullptr, b3, (long long*)nullptr, (long long*)nullptr, S + 1, s));
        if (const int rc = slots_reserve(h, M->L, std::max(b2, b3))) return rc;
        const size_t S1 = (size_t)S + 1;
        CK(group_realloc(M->n, n, M->nsub, n, M->rank0, n, M->lbp, n, M->rank_of, S, M->fr, n, M->sub, S, M->rec, S, M->A, S1, M->A2, S1, M->PA, S1,
                         M->PA2, S1, M->cover, words, M->nbad, 1));
        M->S = S;
    }
    CK(M->win.reserve_grow(5 * (size_t)n_win));
    // the origins in the caller's order, and sorted by row origin for the contacts' search
    std::vector<int> hw(5 * (size_t)n_win), order((size_t)n_win);
    for (int w = 0; w < n_win; w++) { hw[(size_t)w] = origin[2 * w]; hw[(size_t)n_win + w] = origin[2 * w + 1]; order[(size_t)w] = w; }
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        if (origin[2 * a] != origin[2 * b]) return origin[2 * a] < origin[2 * b];
        if (origin[2 * a + 1] != origin[2 * b + 1]) return origin[2 * a + 1] < origin[2 * b + 1];
        return a < b;
    });
    for (int w = 0; w < n_win; w++) {
        const int o = order[(size_t)w];
        hw[2 * (size_t)n_win + w] = origin[2 * o]; hw[3 * (size_t)n_win + w] = origin[2 * o + 1]; hw[4 * (size_t)n_win + w] = o;
    }
    const int *u0 = M->win, *v0 = M->win + n_win, *su0 = M->win + 2 * (size_t)n_win, *sv0 = M->win + 3 * (size_t)n_win,
              *simg = M->win + 4 * (size_t)n_win;
    LayoutSlots& L = M->L;
    const SoaPtr sp = h->soa[h->cur];
    int rc = GRAAL_OK;
    unsigned err = 0;
    unsigned long long nbad = 0;
    do {
        STEP_CK(hipMemcpyAsync(M->win, hw.data(), sizeof(int) * hw.size(), hipMemcpyHostToDevice, s));
        STEP_CK(hipMemsetAsync(M->nbad, 0, sizeof(unsigned long long), s));
        STEP_CK(hipMemsetAsync(M->nsub, 0, sizeof(int) * (size_t)n, s));
        STEP_CK(hipMemsetAsync(M->lbp, 0, sizeof(int) * (size_t)n, s));
        STEP_CK(hipMemsetAsync(M->fr, 0, sizeof(JnFrag) * (size_t)n, s));       // (a slot no fragment claims -- a corrupt layout -- reads as empty)
        STEP_CK(hipMemsetAsync(M->rank_of, 0xff, sizeof(int) * (size_t)S, s));  // (-1: a sub-fragment no slot ranks is left out)
        STEP_CK(hipMemsetAsync(M->rec, 0, sizeof(MwRec) * (size_t)S, s));
        STEP_CK(hipMemsetAsync(M->A, 0, sizeof(long long) * ((size_t)S + 1), s));
        STEP_CK(hipMemsetAsync(M->A2, 0, sizeof(long long) * ((size_t)S + 1), s));
        STEP_CK(hipMemsetAsync(M->cover, 0, sizeof(unsigned) * (size_t)words, s));
        STEP_CK(hipMemsetAsync(M->O, 0, sizeof(long long) * px, s));
        if ((rc = slots_count(h, L))) break;
        k_jn_prep<<<blocks_for(n, 256), 256, 0, s>>>(sp, n, h->stat_frag, h->d_sub_ids, L.cnt, L.base, L.slot, M->fr, M->sub, L.err);
        STEP_CK(hipGetLastError());
        k_mp_slots<<<blocks_for(n, 256), 256, 0, s>>>(sp, n, L.slot, h->stat_frag, M->nsub, M->lbp, L.err);
        STEP_CK(hipGetLastError());
        if ((rc = slots_read_err(h, L, err)) || err) break;   // (a corrupt layout or an inactive fragment)
        size_t tb = L.tmp.count;
        STEP_CK(hipcub::DeviceScan::ExclusiveSum(L.tmp.p, tb, M->nsub.p, M->rank0.p, n, s));
        // (at bin 1 a pixel is a rank: pix is rank_of_sub, A and A2 are the RF count and its square per rank)
        k_mp_rank<<<blocks_for(n, 256), 256, 0, s>>>(n, S, 1, M->fr, M->nsub, M->rank0, h->d_sub_ids, M->rank_of, M->A, M->A2, L.err);
        STEP_CK(hipGetLastError());
        if ((rc = slots_read_err(h, L, err)) || err) break;   // (the ranks do not cover the sub-fragments: no pixel is to be trusted)
        tb = L.tmp.count;
        STEP_CK(hipcub::DeviceScan::ExclusiveSum(L.tmp.p, tb, M->A.p, M->PA.p, S + 1, s));
        tb = L.tmp.count;
        STEP_CK(hipcub::DeviceScan::ExclusiveSum(L.tmp.p, tb, M->A2.p, M->PA2.p, S + 1, s));
        k_mw_rec<<<blocks_for(n, 256), 256, 0, s>>>(n, S, M->fr, M->rank0, M->lbp, M->rec);
        STEP_CK(hipGetLastError());
        if (h->nnz > 0) {
            k_mw_cover<<<blocks_for(2ll * n_win, 256), 256, 0, s>>>(n_win, u0, v0, px_rows, px_cols, bin, S, M->cover);
            STEP_CK(hipGetLastError());
            const size_t bm_bytes = sizeof(unsigned) * (size_t)words;
            const int in_lds = bm_bytes <= MW_LDS_BITMAP_BYTES ? 1 : 0;
            k_mw_obs<<<stream_blocks(h->nnz), 256, in_lds ? bm_bytes : 0, s>>>(h->row, h->col, h->cnt, h->nnz, M->rank_of, M->cover, words, in_lds,
                                                                              n_win, su0, sv0, simg, px_rows, px_cols, bin, M->O);
            STEP_CK(hipGetLastError());
        }
        if (bin <= MW_THREAD_BIN)
            k_mw_exp_t<<<blocks_for((long long)px, 256), 256, 0, s>>>(n_win, u0, v0, px_rows, px_cols, bin, S, M->rec, h->nfpb, h->par, reach_bp(h),
                                                                     M->E, M->badf);
        else {
            const int run = std::max(1, MW_TILE / bin), runs = (px_cols + run - 1) / run;
            k_mw_exp_w<<<(unsigned)((long long)n_win * px_rows * runs), 256, 0, s>>>(n_win, u0, v0, px_rows, px_cols, bin, S, run, runs, M->rec,
                                                                                    h->nfpb, h->par, reach_bp(h), M->E, M->badf);
        }
        STEP_CK(hipGetLastError());
        const double v = h->par.v_inter < 0.0f ? 0.0 : (double)h->par.v_inter;   // (a negative expected value counts as 0)
        k_mw_out<<<blocks_for((long long)px, 256), 256, 0, s>>>(n_win, u0, v0, px_rows, px_cols, bin, S, M->O, M->E, M->badf, M->PA, M->PA2,
                                                                v / (double)h->nfpb, M->obs, M->exp, M->res, M->nbad);
        STEP_CK(hipGetLastError());
        STEP_CK(hipMemcpyAsync(&nbad, M->nbad, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    if (!rc && (err & 16u))
        return fail(h, GRAAL_E_UNSUPPORTED, "graal_map_windows: the layout holds an inactive fragment (those arise only with repeated bins)");
    rc = score_exit(h, "graal_map_windows", rc, nullptr, err);
    if (rc) return rc;
    M->n_win = n_win; M->pr = px_rows; M->pc = px_cols; M->valid = true;
    if (bad_pixels_out) *bad_pixels_out = (int64_t)nbad;
    return GRAAL_OK;
}

int graal_map_windows_fetch(graal_ctx* h, float* observed, float* expected, float* residual, int32_t* rank_of_sub)
{
    if (!h) return GRAAL_E_ARG;
    const MwBuf* M = h->mw;
    if (!M || !M->valid) return fail(h, GRAAL_E_STATE, "graal_map_windows_fetch: call graal_map_windows first");
    CK(hipSetDevice(h->device));
    const size_t bytes = sizeof(float) * (size_t)M->n_win * (size_t)M->pr * (size_t)M->pc;
    if (observed) CK(hipMemcpyAsync(observed, M->obs, bytes, hipMemcpyDeviceToHost, h->stream));
    if (expected) CK(hipMemcpyAsync(expected, M->exp, bytes, hipMemcpyDeviceToHost, h->stream));
    if (residual) CK(hipMemcpyAsync(residual, M->res, bytes, hipMemcpyDeviceToHost, h->stream));
    if (rank_of_sub && M->S > 0 && M->n > 0)
        CK(hipMemcpyAsync(rank_of_sub, M->rank_of, sizeof(int32_t) * (size_t)M->S, hipMemcpyDeviceToHost, h->stream));
    CK(hipStreamSynchronize(h->stream));
    return GRAAL_OK;
}

} // extern "C"
