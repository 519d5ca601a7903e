// maps.h -- the observed contacts, the contacts the model expects and their residual as images in the current genome order
// (graal_layout_maps / graal_layout_maps_fetch; semantics in include/graal_hip.h).
// Included by graal_hip.hip after edit.h (it uses score_common.h, map_shape.h, layout_slots.h's LayoutSlots, wave_runs.h's
// run_sums, and junctions.h's records of the slots: k_jn_prep, JnFrag, jn_blank).
//
// Order.  Slots as for the junction scores (contig label -> member count -> exclusive scan -> offset + position: contigs by ascending label,
// fragments by position), built from the layout fields, not from the engine's position index: the call does not relabel.  One more
// exclusive scan, of the sub-fragment count over the slots, gives a slot's first rank; a fragment's sub-fragments follow in stored order,
// reversed when ori == -1.  Rank u lies in pixel u / bin (map_shape.h).
//
// Kernels, all on the engine's stream:
//   slots_count (k_jn_count / scan) / k_jn_prep / k_mp_slots / scan / k_mp_rank -- slots, ranks, pixel_of_sub, and per pixel the sum of the RF counts and of
//                their squares (int64, exact);
//   k_mp_obs  -- streams the contact list, 64 consecutive contacts per wave; count * 2^24 rounded once, summed per run of equal pixels inside
//                the wave (run_sums), one int64 atomic per run into the upper triangle;
//   k_mp_cis  -- k_full_mass_t's windowed tiling over the slots: for every cis sub-fragment pair inside the window of a linear contig, and
//                every pair of a circular one, max(cis, 0) - max(trans, 0) of the two float32 prices in Q30, rounded once per pair; beyond
//                the window the two prices are the same float32 value and the pair is skipped.  With bin > 1 neighbouring lanes hit the same
//                pixel: runs of equal pixels are summed inside the wave before the atomic.  A term that is not finite or does not fit sets
//                its pixel's bit in a bitmap;
//   k_mp_out  -- per pixel of the m x m images: observed and expected from the two int64 sums of the upper triangle (mirrored; the diagonal
//                twice), the background max(v_inter, 0) / nfpb * A_p * A_q in float64 from the exact integers, the residual.
// A circular contig costs O(len^2) pairs: rings are few.
#pragma once

namespace {

constexpr double MP_O_SCALE = 16777216.0;   // 2^24: the fixed point of the observed sums

struct MpTile { int start_bp, n, r0, fwd; float c0, c1, c2; int a0, a1, a2, pad0, pad1; };   // one staged slot, 48 bytes

struct MpBuf {
    int n = 0, S = 0;                         // the layout buffers' sizes
    LayoutSlots L;                            // (its tmp also serves the scan of nsub)
    DevBuf<int> nsub, rank0, lbp, pix;
    DevBuf<JnFrag> fr;
    DevBuf<JnSub> sub;
    DevBuf<long long> A, A2;                  // per pixel: sum of RF counts, sum of their squares
    DevBuf<unsigned long long> nbad;
    size_t px_cap = 0;                        // pixels the image buffers hold (they only grow)
    DevBuf<long long> O, E;
    DevBuf<unsigned> badmap;
    DevBuf<float> obs, exp, res;
    int m = 0, bin = 1;
    bool valid = false;                       // the images are those of a finished call
};

void mp_free(MpBuf* b) { delete b; }

// per fragment: its slot's sub-fragment count and contig length; an inactive fragment is flagged (err bit 4)
__global__ void k_mp_slots(SoaPtr s, int n, const int* __restrict__ slot_of, const Stat* __restrict__ stat, int* __restrict__ nsub,
                           int* __restrict__ lbp, unsigned* __restrict__ err)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    if (s.p[F_ACTIV][f] != 1) atomicOr(err, 16u);
    const int k = slot_of[f];
    if (k < 0) return;
    nsub[k] = stat[f].n;
    lbp[k] = s.p[F_LCONTBP][f];
}

// per slot: the pixel of each of its sub-fragments, and the pixels' RF-count sums.  err bit 3: the ranks do not add up to S, or an id is out of range
__global__ void k_mp_rank(int n, int S, int bin, const JnFrag* __restrict__ fr, const int* __restrict__ nsub, const int* __restrict__ rank0,
                          const int* __restrict__ sub_ids, int* __restrict__ pix, long long* __restrict__ A, long long* __restrict__ A2,
                          unsigned* __restrict__ err)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const JnFrag r = fr[i];
    const int r0 = rank0[i];
    if (i == n - 1 && r0 + nsub[i] != S) atomicOr(err, 8u);
    if (r.n != nsub[i] || r0 < 0 || r0 + r.n > S) { if (r.n != nsub[i]) atomicOr(err, 8u); return; }
    int4 ids = make_int4(r.frag, 0, 0, 1);
    if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[r.frag];
    for (int k = 0; k < r.n; k++) {
        const int id = sel3(ids.x, ids.y, ids.z, k);
        if (id < 0 || id >= S) { atomicOr(err, 8u); continue; }
        const int p = map_pixel(r0 + ((r.flags & 1) ? k : r.n - 1 - k), bin);
        const long long a = sel3(r.a0, r.a1, r.a2, k);
        pix[id] = p;
        atomicAdd((unsigned long long*)&A[p], (unsigned long long)a);
        atomicAdd((unsigned long long*)&A2[p], (unsigned long long)(a * a));
    }
}

__global__ __launch_bounds__(256) void k_mp_obs(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt, long long nnz,
                                                const int* __restrict__ pix, int m, long long* __restrict__ O)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {   // (wave-uniform bounds: run_sums needs the whole wave)
        const long long k = k0 + lane;
        int key = -1;
        long long v = 0;
        if (k < nnz) {
            const int r = row[k], c = col[k];
            if (r != c) {
                const int pr = pix[r], pc = pix[c];
                if (pr >= 0 && pc >= 0) {
                    key = min(pr, pc) * m + max(pr, pc);
                    v = __double2ll_rn((double)__int_as_float(cnt[k]) * MP_O_SCALE);
                }
            }
        }
        bool tail;
        run_sums(key, tail, v);
        if (tail && key >= 0 && v != 0) atomicAdd((unsigned long long*)&O[key], (unsigned long long)v);
    }
}

// One term into the upper triangle's sums.  Whole wave; key -1: no term in this lane.
__device__ __forceinline__ void mp_add(bool merge, int key, long long q, long long* __restrict__ E, unsigned* __restrict__ badmap)
{
    if (key >= 0 && q == Q_BAD) { atomicOr(&badmap[key >> 5], 1u << (key & 31)); key = -1; }
    if (key < 0) q = 0;
    if (merge) {
        bool tail;
        run_sums(key, tail, q);
        if (!tail) key = -1;
    }
    if (key >= 0 && q != 0) atomicAdd((unsigned long long*)&E[key], (unsigned long long)q);
}

// max(cis price, 0) - max(trans price, 0) of one sub-fragment pair in Q30 (a NaN price stays NaN: Q_BAD)
__device__ __forceinline__ long long mp_pair_q(float ca, float cb, int aa, int ab, bool circ, float s_tot, float nfpb, const Par& par)
{
    const float norm = (float)(aa * ab) / nfpb;
    const float sd = fabsf(cb - ca);
    const float ex = (circ ? rippe_circ(sd, s_tot, par) : rippe(sd, par)) * norm;
    const float et = par.v_inter * norm;
    return to_q((double)(ex < 0.0f ? 0.0f : ex) - (double)(et < 0.0f ? 0.0f : et));
}

__device__ __forceinline__ int mp_key(int ra, int rb, int bin, int m)
{
    const int pa = map_pixel(ra, bin), pb = map_pixel(rb, bin);
    return min(pa, pb) * m + max(pa, pb);
}

__global__ __launch_bounds__(256) void k_mp_cis(int n, const JnFrag* __restrict__ fr, const int* __restrict__ rank0, const int* __restrict__ lbp_of,
                                                float nfpb, Par par, int reach_bp, int S, int bin, int m, long long* __restrict__ E,
                                                unsigned* __restrict__ badmap)
{
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int W = blockIdx.x * 4 + wib, tile = W / S, s = W - tile * S;
    __shared__ MpTile s_y[4][64];
    MpTile* const ty = s_y[wib];
    const bool merge = bin > 1;
    const int i = tile * 64 + lane;
    JnFrag x = jn_blank();
    int xr0 = 0;
    float s_tot = 1.0f;
    if (i < n) { x = fr[i]; x.last = min(x.last, n - 1); xr0 = rank0[i]; s_tot = (float)lbp_of[i] / 1000.0f; }
    const bool circ = (x.flags & 2) != 0, xfwd = (x.flags & 1) != 0;
    const int x_end = x.start_bp + x.len_bp;
    if (s == 0) {   // x's own sub-fragment pairs
        for (int a = 0; a < 2; a++)
            for (int b = a + 1; b < 3; b++) {
                const bool on = i < n && b < x.n;
                if (__ballot(on) == 0ull) continue;
                int key = -1;
                long long q = 0;
                if (on) {
                    q = mp_pair_q(sel3(x.c0, x.c1, x.c2, a), sel3(x.c0, x.c1, x.c2, b), sel3(x.a0, x.a1, x.a2, a), sel3(x.a0, x.a1, x.a2, b), circ,
                                  s_tot, nfpb, par);
                    key = mp_key(xr0 + (xfwd ? a : x.n - 1 - a), xr0 + (xfwd ? b : x.n - 1 - b), bin, m);
                }
                mp_add(merge, key, q, E, badmap);
            }
    }
    bool live = i < n && x.last > i;          // (start_bp grows along a contig: once a y of x's contig is beyond the window, all later ones are)
    for (int c = s; ; c += S) {
        const int j0 = tile * 64 + 64 * c;
        if (__ballot(live && x.last >= j0) == 0ull) break;
        {
            const int j = j0 + lane;
            MpTile y;
            y.start_bp = 0; y.n = 0; y.r0 = 0; y.fwd = 0; y.c0 = y.c1 = y.c2 = 0.0f; y.a0 = y.a1 = y.a2 = 0; y.pad0 = y.pad1 = 0;
            if (j < n) {
                const JnFrag g = fr[j];
                y.start_bp = g.start_bp; y.n = g.n; y.r0 = rank0[j]; y.fwd = g.flags & 1; y.c0 = g.c0; y.c1 = g.c1; y.c2 = g.c2;
                y.a0 = g.a0; y.a1 = g.a1; y.a2 = g.a2;
            }
            ty[lane] = y;
        }
        WAVE_LDS_SYNC();
        const int cnt = min(64, n - j0);
        for (int jj = 0; jj < cnt; jj++) {    // (every lane reads the same y: the lanes' pixels differ by x alone, runs of equal pixels are long)
            const int j = j0 + jj;
            const MpTile y = ty[jj];
            bool act = live && j > i && j <= x.last;          // every unordered pair once; x's contig only
            if (act && !circ && y.start_bp - x_end > reach_bp) { live = false; act = false; }   // beyond the window: cis = trans exactly
            if (__ballot(act) == 0ull) continue;
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    const bool on = act && a < x.n && b < y.n;
                    if (__ballot(on) == 0ull) continue;
                    int key = -1;
                    long long q = 0;
                    if (on) {
                        q = mp_pair_q(sel3(x.c0, x.c1, x.c2, a), sel3(y.c0, y.c1, y.c2, b), sel3(x.a0, x.a1, x.a2, a), sel3(y.a0, y.a1, y.a2, b),
                                      circ, s_tot, nfpb, par);
                        key = mp_key(xr0 + (xfwd ? a : x.n - 1 - a), y.r0 + (y.fwd ? b : y.n - 1 - b), bin, m);
                    }
                    mp_add(merge, key, q, E, badmap);
                }
        }
        WAVE_LDS_SYNC();                      // (the next tile is staged over this one)
    }
}

// One pixel from its sums (k_mp_out, and map_windows.h's k_mw_out: the same float64 operations): observed and expected from the two int64
// sums -- `twice` is 2 where the sums hold every pair once and the pixel holds it both ways, else 1 -- the background v_over_nfpb * pairs,
// the residual.  A pixel with a flagged term or a value that is not finite is NaN in expected and residual; returns whether it is.
__device__ __forceinline__ bool mp_pixel(long long o_sum, long long e_sum, double twice, double pairs, double v_over_nfpb, bool flagged,
                                         float& obs, float& exp_, float& res)
{
    const double o = twice * ((double)o_sum / MP_O_SCALE);
    double e = v_over_nfpb * pairs + twice * ((double)e_sum / Q_SCALE);
    const bool bad = flagged || !(fabs(e) < INFINITY);
    double r = 0.0;
    if (bad) { e = (double)NAN; r = (double)NAN; }
    else if (e > 0.0) r = (o - e) / sqrt(e);
    obs = (float)o;
    exp_ = (float)e;
    res = (float)r;
    return bad;
}

__global__ __launch_bounds__(256) void k_mp_out(int m, const long long* __restrict__ O, const long long* __restrict__ E, const unsigned* __restrict__ badmap,
                                                const long long* __restrict__ A, const long long* __restrict__ A2, double v_over_nfpb,
                                                float* __restrict__ obs, float* __restrict__ exp_, float* __restrict__ res,
                                                unsigned long long* __restrict__ nbad)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)m * m) return;
    const int p = (int)(idx / m), q = (int)(idx - (long long)p * m);
    const int key = min(p, q) * m + max(p, q);
    const double twice = p == q ? 2.0 : 1.0;
    const long long ap = A[p], aq = A[q];
    double pairs;   // sum of accu_a accu_b over the pixel's pairs (a diagonal pixel: both ways, as the observed counts)
    if (p != q) pairs = (double)ap * (double)aq;
    else pairs = ap < (1ll << 31) ? (double)(ap * ap - A2[p]) : (double)ap * (double)ap - (double)A2[p];
    float of, ef, rf;
    if (mp_pixel(O[key], E[key], twice, pairs, v_over_nfpb, ((badmap[key >> 5] >> (key & 31)) & 1u) != 0, of, ef, rf)) atomicAdd(nbad, 1ull);
    obs[idx] = of;
    exp_[idx] = ef;
    res[idx] = rf;
}

} // namespace

extern "C" {

int graal_layout_maps(graal_ctx* h, int32_t max_px, int32_t* m_out, int32_t* bin_out, int64_t* bad_pixels_out)
{
    if (!h) return GRAAL_E_ARG;
    if (max_px < 1 || max_px > GRAAL_MAPS_MAX_PX) return fail(h, GRAAL_E_ARG, "graal_layout_maps: max_px must lie in 1 .. 4096");
    if (const int rc = score_entry(h, "graal_layout_maps")) return rc;
    const int n = h->n, S = h->n_sub_total;
    if (!h->mp) h->mp = new MpBuf();
    MpBuf* M = h->mp;
    M->valid = false;
    const MapShape shape = map_shape(std::max(S, 0), max_px);
    const int m = shape.m, bin = shape.bin;
    if (m_out) *m_out = m;
    if (bin_out) *bin_out = bin;
    if (bad_pixels_out) *bad_pixels_out = 0;
    if (n < 1 || S < 1) { M->m = 0; M->bin = 1; M->valid = true; if (m_out) *m_out = 0; return GRAAL_OK; }
    hipStream_t s = h->stream;
    if (M->n != n || M->S != S) {
        size_t b2 = 0;
        CK(hipcub::DeviceScan::ExclusiveSum(nullptr, b2, (int*)nullptr, (int*)nullptr, n, s));
        if (const int rc = slots_reserve(h, M->L, b2)) return rc;
        CK(group_realloc(M->n, n, M->nsub, n, M->rank0, n, M->lbp, n, M->pix, S, M->fr, n, M->sub, S, M->A, S /* m <= S */, M->A2, S, M->nbad, 1));
        M->S = S;
    }
    const size_t px = (size_t)m * (size_t)m, bad_words = (px + 31) / 32;
    CK(group_grow(M->px_cap, px, M->O, px, M->E, px, M->badmap, bad_words, M->obs, px, M->exp, px, M->res, px));
    LayoutSlots& L = M->L;
    const SoaPtr sp = h->soa[h->cur];
    int rc = GRAAL_OK;
    unsigned err = 0;
    unsigned long long nbad = 0;
    do {
        STEP_CK(hipMemsetAsync(M->nbad, 0, sizeof(unsigned long long), s));
        STEP_CK(hipMemsetAsync(M->nsub, 0, sizeof(int) * (size_t)n, s));
        STEP_CK(hipMemsetAsync(M->lbp, 0, sizeof(int) * (size_t)n, s));
        STEP_CK(hipMemsetAsync(M->fr, 0, sizeof(JnFrag) * (size_t)n, s));   // (a slot no fragment claims -- a corrupt layout -- reads as empty)
        STEP_CK(hipMemsetAsync(M->pix, 0xff, sizeof(int) * (size_t)S, s));  // (-1: a sub-fragment no slot ranks is left out)
        STEP_CK(hipMemsetAsync(M->A, 0, sizeof(long long) * (size_t)m, s));
        STEP_CK(hipMemsetAsync(M->A2, 0, sizeof(long long) * (size_t)m, s));
        STEP_CK(hipMemsetAsync(M->O, 0, sizeof(long long) * px, s));
        STEP_CK(hipMemsetAsync(M->E, 0, sizeof(long long) * px, s));
        STEP_CK(hipMemsetAsync(M->badmap, 0, sizeof(unsigned) * bad_words, s));
        if ((rc = slots_count(h, L))) break;
        k_jn_prep<<<blocks_for(n, 256), 256, 0, s>>>(sp, n, h->stat_frag, h->d_sub_ids, L.cnt, L.base, L.slot, M->fr, M->sub, L.err);
        STEP_CK(hipGetLastError());
        k_mp_slots<<<blocks_for(n, 256), 256, 0, s>>>(sp, n, L.slot, h->stat_frag, M->nsub, M->lbp, L.err);
        STEP_CK(hipGetLastError());
        if ((rc = slots_read_err(h, L, err)) || err) break;   // (a corrupt layout or an inactive fragment)
        size_t tb = L.tmp.count;
        STEP_CK(hipcub::DeviceScan::ExclusiveSum(L.tmp.p, tb, M->nsub.p, M->rank0.p, n, s));
        k_mp_rank<<<blocks_for(n, 256), 256, 0, s>>>(n, S, bin, M->fr, M->nsub, M->rank0, h->d_sub_ids, M->pix, M->A, M->A2, L.err);
        STEP_CK(hipGetLastError());
        if ((rc = slots_read_err(h, L, err)) || err) break;   // (the ranks do not cover the sub-fragments: no pixel is to be trusted)
        if (h->nnz > 0) {
            k_mp_obs<<<stream_blocks(h->nnz), 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, M->pix, m, M->O);
            STEP_CK(hipGetLastError());
        }
        const int lc = std::min(std::max(std::max(h->max_lcont, h->lcont_bound), 1), n);
        const int n_tiles = (n + 63) / 64;
        const int Sw = mass_stripes(lc);
        k_mp_cis<<<(n_tiles * Sw + 3) / 4, 256, 0, s>>>(n, M->fr, M->rank0, M->lbp, h->nfpb, h->par, reach_bp(h), Sw, bin, m, M->E, M->badmap);
        STEP_CK(hipGetLastError());
        const double v = h->par.v_inter < 0.0f ? 0.0 : (double)h->par.v_inter;   // (a negative expected value counts as 0)
        k_mp_out<<<blocks_for((long long)px, 256), 256, 0, s>>>(m, M->O, M->E, M->badmap, M->A, M->A2, v / (double)h->nfpb, M->obs, M->exp, M->res,
                                                                 M->nbad);
        STEP_CK(hipGetLastError());
        STEP_CK(hipMemcpyAsync(&nbad, M->nbad, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    if (!rc && (err & 16u))
        return fail(h, GRAAL_E_UNSUPPORTED, "graal_layout_maps: the layout holds an inactive fragment (those arise only with repeated bins)");
    rc = score_exit(h, "graal_layout_maps", rc, nullptr, err);
    if (rc) return rc;
    M->m = m; M->bin = bin; M->valid = true;
    if (bad_pixels_out) *bad_pixels_out = (int64_t)nbad;
    return GRAAL_OK;
}

int graal_layout_maps_fetch(graal_ctx* h, float* observed, float* expected, float* residual, int32_t* pixel_of_sub)
{
    if (!h) return GRAAL_E_ARG;
    const MpBuf* M = h->mp;
    if (!M || !M->valid) return fail(h, GRAAL_E_STATE, "graal_layout_maps_fetch: call graal_layout_maps first");
    if (M->m < 1) return GRAAL_OK;
    CK(hipSetDevice(h->device));
    const size_t bytes = sizeof(float) * (size_t)M->m * (size_t)M->m;
    if (observed) CK(hipMemcpyAsync(observed, M->obs, bytes, hipMemcpyDeviceToHost, h->stream));
    if (expected) CK(hipMemcpyAsync(expected, M->exp, bytes, hipMemcpyDeviceToHost, h->stream));
    if (residual) CK(hipMemcpyAsync(residual, M->res, bytes, hipMemcpyDeviceToHost, h->stream));
    if (pixel_of_sub) CK(hipMemcpyAsync(pixel_of_sub, M->pix, sizeof(int32_t) * (size_t)M->S, hipMemcpyDeviceToHost, h->stream));
    CK(hipStreamSynchronize(h->stream));
    return GRAAL_OK;
}

} // extern "C"
