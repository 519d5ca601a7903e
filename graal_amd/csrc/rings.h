// rings.h -- the likelihood closing each linear contig into a ring, or opening each ring at its wrap, would add, for every contig in one
// pass (graal_ring_scores); and the commit that closes contigs (graal_close_rings).
// Included by graal_hip.hip after junctions.h (it uses Ctx, Stat, rippe, to_q, WAVE_LDS_SYNC, model_math.h, score_common.h's score_entry,
// layout_refusal, score_exit, STEP_CK, stream_blocks, mass_stripes and layout_replaced, layout_slots.h's LayoutSlots and
// slot_claim, wave_runs.h's run_sums, and junctions.h's jn_load).
//
// R[c] = logL(layout with contig c in the OTHER topology, every coordinate kept) - logL(layout), in the engine's exact arithmetic.  Nothing
// moves, so only the price of c's own pairs changes, and only where the two topologies are priced apart: rippe_circ (graal_hip.hip)
// differs from rippe for the pairs whose LINEAR centre distance s lies in (0, d_max) -- there it is rippe(s) * val(n) / norm_circ with
// n = K s (s_tot - s) / s_tot -- and is v_inter like rippe everywhere else.  That is the reference's ring model (kernels3.cu:135-160) and
// its limit: a contig shorter than d_max gets a true ring price, symmetric in s and s_tot - s; in a longer one only the pairs inside the
// window change, and head-tail contacts more than d_max apart along the contig carry nothing.  The score is what graal_eval_full_q
// prices, nothing better.
//   a contact:              ob * (ln ex_new - ln ex_old), rounded to Q once per contact (two sub-fragments of one bin included);
//   a fragment pair's mass: -(sum over its sub-fragment pairs of ex_new - ex_old) in float64, rounded to Q once per fragment pair; a bin's
//                           own sub-fragment pairs (a < b) count as one such pair.
// GRAAL_MODE_REF_TRANS_ACCU does not enter: it re-indexes trans prices only, and a cis pair beyond the window is v_inter * the plain norm
// in both topologies.
//
// The slot numbering is layout_slots.h's, built from the layout itself (slots_count -> k_rg_prep): the call does not relabel and leaves
// the step state alone.  A contig is keyed by its LAST slot.  Kernels, all on the engine's stream:
//   k_rg_prep -- a 48-byte record per slot and a 16-byte record per sub-fragment (both carry the contig's key and s_tot; rings are scored
//                here, so the junction scorer's records, which mark rings out, do not serve); the longest contig of THIS layout, which
//                sizes k_rg_mass's grid (the handle's own statistic is that of its last graal_begin_step);
//   k_rg_nnz  -- streams the contact list, 64 consecutive contacts per wave, each keyed by its row's contig; the terms, the wrap-side counts
//                and the bad terms are summed per run of equal keys inside the wave, one 64-bit atomic per run and sum;
//   k_rg_mass -- k_jn_mass's tiling: a wave's lanes are 64 consecutive slots x, the slots y behind them staged in LDS 64 at a time, S waves
//                per x tile, the window exit (reach_bp) kept.  A lane needs its row sum only: every lane reads the same staged y at each
//                step (an LDS broadcast), no column sums, no hand-off between steps; one segmented wave sum by contig and one atomic per
//                run at the end.  A bin's own pairs are added by the bin's lane in the tile's first wave;
//   k_rg_out  -- the per-fragment outputs.
// Compiler's figures (gfx950, -O3): k_rg_nnz 77 VGPRs, k_rg_mass 91 VGPRs and 12 KB of LDS per block, no scratch in any of them.
// norm_circ and powf(kuhn, -3) of rippe_circ depend on the parameters only: RgPre holds them, computed once per thread by the same
// operations in the same order, so every price is the float32 rippe_circ returns; per pair that leaves rippe, one powf and one expf.
//
// graal_close_rings is one kernel of one block: validate the named fragments, count the names per contig, find heads and tails, and only
// when nothing is refused write circ, the head's prev and the tail's next.
#pragma once

namespace {

struct RgSub { int key; float centre; int accu; float s_tot; };   // key: the contig's last slot; accu: RF count | ring << 16
struct RgFrag { int start_bp, len_bp, flags, n; int a0, a1, a2, last; float c0, c1, c2, s_tot; };   // per slot; flags bit0 fwd, bit1 ring
struct RgPre { float K, k3, norm_circ; };

struct RgBuf {
    int n = 0, S = 0;
    LayoutSlots L;                                              // (err[1]: the longest contig)
    DevBuf<RgFrag> fr;
    DevBuf<RgSub> sub;
    DevBuf<long long> sum; long long *con = nullptr, *bad = nullptr;   // per slot, used at a contig's last slot (one allocation of 3n)
    DevBuf<long long> q, c; DevBuf<unsigned char> st;           // the results, fragment-indexed
    DevBuf<int> mark, head, tail, d_frag, d_st; int n_lab = 0, fcap = 0;   // graal_close_rings
};

void rg_free(RgBuf* b) { delete b; }

// the parameter-only factors of rippe_circ, by its own operations
__device__ __forceinline__ RgPre rg_pre(const Par& p)
{
    RgPre r;
    r.K = p.lm / p.kuhn;
    const float nmax = r.K * 1;
    r.k3 = mm_powf(p.kuhn, -3.0f);
    r.norm_circ = (r.k3 * mm_powf(nmax, p.slope) * mm_expf((p.d - 2.0f) / (sq(nmax) + p.d))) * p.fact;
    return r;
}

// rippe_circ(s, s_tot, p) for 0 < s < d_max, given lin = rippe(s, p)
__device__ __forceinline__ float rg_circ(float s, float s_tot, float lin, const RgPre& c, const Par& p)
{
    const float n = c.K * s * (s_tot - s) / s_tot;
    const float val = (c.k3 * mm_powf(n, p.slope) * mm_expf((p.d - 2.0f) / (sq(n) + p.d))) * p.fact;
    return fmaxf(val * lin / c.norm_circ, p.v_inter);
}

// ex_new - ex_old of one sub-fragment pair at linear distance sd; exactly 0 outside (0, d_max)
__device__ __forceinline__ double rg_pair_diff(float sd, float s_tot, int prod, bool ring, float nfpb, const RgPre& c, const Par& p)
{
    if (!(sd > 0.0f && sd < p.d_max)) return 0.0;
    const float norm = (float)prod / nfpb;
    const float lin = rippe(sd, p);
    const float ex_lin = lin * norm, ex_circ = rg_circ(sd, s_tot, lin, c, p) * norm;
    return ring ? (double)ex_lin - (double)ex_circ : (double)ex_circ - (double)ex_lin;
}

__global__ __launch_bounds__(256) void k_rg_prep(SoaPtr s, int n, const Stat* __restrict__ stat, const int* __restrict__ sub_ids,
                                                 const int* __restrict__ cnt, const int* __restrict__ base, int* __restrict__ slot_of,
                                                 RgFrag* __restrict__ fr, RgSub* __restrict__ sub, unsigned* __restrict__ err)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int slot = slot_claim(s, n, f, cnt, base, slot_of, &err[0]);
    if (slot < 0) return;
    const int c = s.p[F_IDC][f];
    if (s.p[F_POS][f] == 0) atomicMax(&err[1], (unsigned)cnt[c]);
    const JnLoad x = jn_load(s, stat, f);
    const Stat& st = x.st;
    const bool ring = x.circ;
    RgFrag r;
    r.start_bp = x.start; r.len_bp = x.len; r.flags = (x.fwd ? 1 : 0) | (ring ? 2 : 0);
    r.n = st.n; r.a0 = st.a0; r.a1 = st.a1; r.a2 = st.a2;
    r.c0 = x.c0; r.c1 = x.c1; r.c2 = x.c2;
    r.last = min(base[c] + cnt[c] - 1, n - 1);
    r.s_tot = (float)s.p[F_LCONTBP][f] / 1000.0f;
    fr[slot] = r;
    int4 ids = make_int4(f, 0, 0, 1);
    if (sub_ids) ids = reinterpret_cast<const int4*>(sub_ids)[f];
    for (int k = 0; k < st.n; k++) {
        RgSub u;
        u.key = r.last;
        u.centre = sel3(r.c0, r.c1, r.c2, k);
        u.accu = stat_accu(st, k) | ((ring ? 1 : 0) << 16);   // (RF counts are <= 30000)
        u.s_tot = r.s_tot;
        sub[sel3(ids.x, ids.y, ids.z, k)] = u;
    }
}

__global__ __launch_bounds__(256) void k_rg_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt,
                                                long long nnz, const RgSub* __restrict__ sub, float nfpb, Par par,
                                                long long* __restrict__ sum, long long* __restrict__ con, long long* __restrict__ bad)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    const RgPre pre = rg_pre(par);
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {   // (wave-uniform bounds: run_sums needs the whole wave)
        const long long k = k0 + lane;
        int key = -1;
        long long vq = 0, vc = 0, vb = 0;
        if (k < nnz) {
            const RgSub A = sub[row[k]], B = sub[col[k]];
            key = A.key;                                             // (the row's contig: a row's contacts form one run)
            const float sd = fabsf(B.centre - A.centre);
            if (A.key == B.key && sd > 0.0f && sd < par.d_max) {
                const bool ring = (A.accu >> 16) != 0;
                const float norm = (float)((A.accu & 0xffff) * (B.accu & 0xffff)) / nfpb;
                const float lin = rippe(sd, par);
                const float ex_lin = lin * norm, ex_circ = rg_circ(sd, A.s_tot, lin, pre, par) * norm;
                const double ob = (double)__int_as_float(cnt[k]);
                const long long q = to_q(ob * (mm_ln(ring ? ex_lin : ex_circ) - mm_ln(ring ? ex_circ : ex_lin)));
                if (q == Q_BAD) vb = 1; else vq = q;
                if (2.0f * sd > A.s_tot) vc = (long long)llrint(ob);
            }
        }
        bool t1, t2, t3;
        run_sums(key, t1, vq);
        run_sums(key, t2, vc);
        run_sums(key, t3, vb);
        if (t1 && key >= 0) {
            if (vq != 0) atomicAdd((unsigned long long*)&sum[key], (unsigned long long)vq);
            if (vc != 0) atomicAdd((unsigned long long*)&con[key], (unsigned long long)vc);
            if (vb != 0) atomicAdd((unsigned long long*)&bad[key], (unsigned long long)vb);
        }
    }
}

// -(sum of ex_new - ex_old) over the sub-fragment pairs of x (outer) and y, in Q; Q_BAD if it is not finite or does not fit
__device__ __forceinline__ long long rg_pair_mass(const RgFrag& x, const RgFrag& y, float nfpb, const RgPre& pre, const Par& par)
{
    double acc = 0.0;
    for (int a = 0; a < x.n; a++)
        for (int b = 0; b < y.n; b++)
            acc += rg_pair_diff(fabsf(sel3(y.c0, y.c1, y.c2, b) - sel3(x.c0, x.c1, x.c2, a)), x.s_tot,
                                sel3(x.a0, x.a1, x.a2, a) * sel3(y.a0, y.a1, y.a2, b), x.flags & 2, nfpb, pre, par);
    return to_q_fast(acc);
}

__global__ __launch_bounds__(256) void k_rg_mass(int n, const RgFrag* __restrict__ fr, float nfpb, Par par, int reach_bp, int S,
                                                 long long* __restrict__ sum, long long* __restrict__ bad)
{
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const int W = blockIdx.x * 4 + wib, tile = W / S, s = W - tile * S;
    __shared__ RgFrag s_y[4][64];
    RgFrag* const ty = s_y[wib];
    const int i = tile * 64 + lane;                                  // (a wave past the last tile has no lane below n: it stages nothing)
    const RgPre pre = rg_pre(par);
    RgFrag x;
    x.start_bp = 0; x.len_bp = 0; x.flags = 0; x.n = 0; x.a0 = x.a1 = x.a2 = 0; x.last = -1; x.c0 = x.c1 = x.c2 = 0.0f; x.s_tot = 1.0f;
    if (i < n) x = fr[i];
    const int x_end = x.start_bp + x.len_bp;
    long long row = 0, nb = 0;
    if (s == 0 && i < n && x.n > 1) {                                // the bin's own pairs: one fragment pair, rounded once
        double acc = 0.0;
        for (int a = 0; a < x.n; a++)
            for (int b = a + 1; b < x.n; b++)
                acc += rg_pair_diff(fabsf(sel3(x.c0, x.c1, x.c2, b) - sel3(x.c0, x.c1, x.c2, a)), x.s_tot,
                                    sel3(x.a0, x.a1, x.a2, a) * sel3(x.a0, x.a1, x.a2, b), x.flags & 2, nfpb, pre, par);
        const long long q = to_q_fast(acc);
        if (q == Q_BAD) nb++; else row -= q;
    }
    bool live = i < n && x.last > i;
    for (int c = s; ; c += S) {
        const int j0 = tile * 64 + 64 * c;
        if (__ballot(live && x.last >= j0) == 0ull) break;           // (x.last < n: j0 < n past this line)
        if (j0 + lane < n) ty[lane] = fr[j0 + lane];
        WAVE_LDS_SYNC();
        if (live) {
            const int t1 = min(63, x.last - j0);                     // (x.last >= j0 - 63 always: the tile's own chunk is c = 0)
            for (int t = max(0, i + 1 - j0); t <= t1; t++) {
                const RgFrag& y = ty[t];
                if (y.start_bp - x_end > reach_bp) { live = false; break; }   // beyond the window: both topologies price v_inter * norm
                const long long q = rg_pair_mass(x, y, nfpb, pre, par);
                if (q == Q_BAD) nb++; else row -= q;
            }
        }
        live = live && x.last >= j0 + 64;
        WAVE_LDS_SYNC();                                             // (the next chunk overwrites the staged records)
    }
    const int key = i < n ? x.last : -1;
    bool t1, t2;
    run_sums(key, t1, row);
    run_sums(key, t2, nb);
    if (t1 && key >= 0) {
        if (row != 0) atomicAdd((unsigned long long*)&sum[key], (unsigned long long)row);
        if (nb != 0) atomicAdd((unsigned long long*)&bad[key], (unsigned long long)nb);
    }
}

__global__ void k_rg_out(SoaPtr s, int n, const int* __restrict__ cnt, const int* __restrict__ slot_of, const RgFrag* __restrict__ fr,
                         const long long* __restrict__ sum,
                         const long long* __restrict__ con, const long long* __restrict__ bad, long long* __restrict__ q_out,
                         long long* __restrict__ c_out, unsigned char* __restrict__ st_out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int k = slot_of[f];                                        // (>= 0: a corrupt layout never gets here)
    const int key = fr[k].last;
    const bool ring = s.p[F_CIRC][f] == 1;
    unsigned char st = ring ? GRAAL_RING_OPEN : GRAAL_RING_CLOSE;
    if (!ring && cnt[s.p[F_IDC][f]] < 2) st = GRAAL_RING_SINGLE;
    else if (bad[key] != 0) st = GRAAL_RING_NONFINITE;
    q_out[f] = (st == GRAAL_RING_OPEN || st == GRAAL_RING_CLOSE) ? sum[key] : 0;
    c_out[f] = con[key];
    st_out[f] = st;
}

// graal_close_rings, one block.  mark / head / tail: per contig label, zeroed / -1 / -1 by the host; scal[0]: layout-error flags.
__global__ __launch_bounds__(1024) void k_rg_close(SoaPtr s, int n, int n_lab, int n_rings, const int* __restrict__ frag, int* __restrict__ st,
                                                   int* __restrict__ mark, int* __restrict__ head, int* __restrict__ tail, int* __restrict__ scal)
{
    __shared__ int s_refused, s_err;
    if (threadIdx.x == 0) { s_refused = 0; s_err = 0; }
    __syncthreads();
    for (int k = threadIdx.x; k < n_rings; k += blockDim.x) {
        const int f = frag[k];
        int r = GRAAL_RINGEDIT_OK;
        if (f < 0 || f >= n) r = GRAAL_RINGEDIT_BAD_FRAG;
        else {
            const int c = s.p[F_IDC][f];
            if (c < 0 || c >= n_lab) { r = GRAAL_RINGEDIT_BAD_FRAG; s_err = 1; }
            else if (s.p[F_CIRC][f] == 1) r = GRAAL_RINGEDIT_CIRCULAR;
            else if (s.p[F_LCONT][f] < 2) r = GRAAL_RINGEDIT_SINGLE;
            else atomicAdd(&mark[c], 1);
        }
        st[k] = r;
        if (r != GRAAL_RINGEDIT_OK) s_refused = 1;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_rings; k += blockDim.x)
        if (st[k] == GRAAL_RINGEDIT_OK && mark[s.p[F_IDC][frag[k]]] > 1) { st[k] = GRAAL_RINGEDIT_TWICE; s_refused = 1; }
    __syncthreads();
    if (s_refused || s_err) { if (threadIdx.x == 0 && s_err) scal[0] = 1; return; }
    for (int f = threadIdx.x; f < n; f += blockDim.x) {
        const int c = s.p[F_IDC][f];
        if (c < 0 || c >= n_lab) { s_err = 1; continue; }
        if (mark[c] == 0) continue;
        const int pos = s.p[F_POS][f];
        if (pos == 0 && atomicCAS(&head[c], -1, f) != -1) s_err = 1;
        if (pos == s.p[F_LCONT][f] - 1 && atomicCAS(&tail[c], -1, f) != -1) s_err = 1;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_rings; k += blockDim.x) {
        const int c = s.p[F_IDC][frag[k]];
        if (head[c] < 0 || tail[c] < 0 || head[c] == tail[c]) s_err = 1;
    }
    __syncthreads();
    if (s_err) { if (threadIdx.x == 0) scal[0] = 1; return; }        // (a corrupt layout: nothing was written)
    for (int f = threadIdx.x; f < n; f += blockDim.x) {
        const int c = s.p[F_IDC][f];
        if (mark[c] == 0) continue;
        s.p[F_CIRC][f] = 1;
        if (f == head[c]) s.p[F_PREV][f] = tail[c];
        if (f == tail[c]) s.p[F_NEXT][f] = head[c];
    }
}

} // namespace

extern "C" {

int graal_ring_scores(graal_ctx* h, int64_t* q_out, int64_t* contacts_out, uint8_t* status)
{
    if (!h || !q_out || !contacts_out || !status) return GRAAL_E_ARG;
    if (const int rc = score_entry(h, "graal_ring_scores")) return rc;
    const int n = h->n, S = h->n_sub_total;
    if (n < 1) return GRAAL_OK;
    if (!h->rg) h->rg = new RgBuf();
    RgBuf* R = h->rg;
    hipStream_t s = h->stream;
    if (R->n != n || R->S != S) {
        if (const int rc = slots_reserve(h, R->L)) return rc;
        CK(group_realloc(R->n, n, R->fr, n, R->sub, std::max(S, 1), R->sum, 3 * (size_t)n, R->q, n, R->c, n, R->st, n));
        R->S = S;
    }
    R->con = R->sum + n; R->bad = R->sum + 2 * (size_t)n;
    LayoutSlots& L = R->L;
    const SoaPtr sp = h->soa[h->cur];
    int rc = GRAAL_OK;
    unsigned err = 0, longest = 0;
    do {
        STEP_CK(hipMemsetAsync(R->sum, 0, sizeof(long long) * 3 * (size_t)n, s));
        STEP_CK(hipMemsetAsync(R->fr, 0, sizeof(RgFrag) * (size_t)n, s));   // (a slot no fragment claims -- a corrupt layout -- reads as empty)
        if ((rc = slots_count(h, L))) break;
        k_rg_prep<<<blocks_for(n, 256), 256, 0, s>>>(sp, n, h->stat_frag, h->d_sub_ids, L.cnt, L.base, L.slot, R->fr, R->sub, L.err);
        STEP_CK(hipGetLastError());
        if ((rc = slots_read_err(h, L, err, &longest)) || err) break;
        if (h->nnz > 0) {
            k_rg_nnz<<<stream_blocks(h->nnz), 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, R->sub, h->nfpb, h->par, R->sum, R->con, R->bad);
            STEP_CK(hipGetLastError());
        }
        const int lc = std::min(std::max((int)longest, 1), n);       // the longest contig of the layout scored
        const int n_tiles = (n + 63) / 64;
        const int Sw = mass_stripes(lc);
        k_rg_mass<<<(n_tiles * Sw + 3) / 4, 256, 0, s>>>(n, R->fr, h->nfpb, h->par, reach_bp(h), Sw, R->sum, R->bad);
        STEP_CK(hipGetLastError());
        k_rg_out<<<blocks_for(n, 256), 256, 0, s>>>(sp, n, L.cnt, L.slot, R->fr, R->sum, R->con, R->bad, R->q, R->c, R->st);
        STEP_CK(hipGetLastError());
        STEP_CK(hipMemcpyAsync(q_out, R->q, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(contacts_out, R->c, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipMemcpyAsync(status, R->st, (size_t)n, hipMemcpyDeviceToHost, s));
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    return score_exit(h, "graal_ring_scores", rc, nullptr, err);
}

int graal_close_rings(graal_ctx* h, int32_t n_rings, const int32_t* frag, int32_t* status)
{
    if (!h || n_rings < 0 || (n_rings > 0 && (!frag || !status))) return GRAAL_E_ARG;
    // (the scorers' refusals, but for what must be uploaded: the commit needs neither contacts nor parameters)
    if (const int rc = layout_refusal(h, "graal_close_rings", h->have_frags ? nullptr : "upload the fragments first")) return rc;
    for (int i = 0; i < n_rings; i++) status[i] = GRAAL_RINGEDIT_OK;
    if (n_rings == 0) return GRAAL_OK;
    CK(hipSetDevice(h->device));
    // (what graal_edit_layout waits for: graal_begin_step's relabel kernels, the last commit's own-pixel correction)
    CK(hipStreamSynchronize(h->stream));
    if (h->fstream) CK(hipStreamSynchronize(h->fstream));
    if (h->own_pending) { const int rc = wait_own(h, nullptr, nullptr); if (rc) return rc; }
    const int n = h->n, NL = 2 * n + 5;   // (labels < 2n + 4, as graal_upload_frags accepts them)
    hipStream_t s = h->stream;
    if (!h->rg) h->rg = new RgBuf();
    RgBuf* R = h->rg;
    if (R->n_lab != NL || n_rings > R->fcap) {
        CK(group_realloc(R->n_lab, NL, R->mark, NL + 1 /* the error word */, R->head, NL, R->tail, NL, R->d_frag, n_rings, R->d_st, n_rings));
        R->fcap = n_rings;
    }
    CK(hipMemcpyAsync(R->d_frag, frag, sizeof(int) * (size_t)n_rings, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(R->d_st, 0, sizeof(int) * (size_t)n_rings, s));
    CK(hipMemsetAsync(R->mark, 0, sizeof(int) * (size_t)(NL + 1), s));
    CK(hipMemsetAsync(R->head, 0xff, sizeof(int) * (size_t)NL, s));
    CK(hipMemsetAsync(R->tail, 0xff, sizeof(int) * (size_t)NL, s));
    k_rg_close<<<1, 1024, 0, s>>>(h->soa[h->cur], n, NL, n_rings, R->d_frag, R->d_st, R->mark, R->head, R->tail, R->mark + NL);
    CK(hipGetLastError());
    std::vector<int> hst((size_t)n_rings);
    int bad_layout = 0;
    CK(hipMemcpyAsync(hst.data(), R->d_st, sizeof(int) * hst.size(), hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&bad_layout, R->mark + NL, sizeof(int), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    for (size_t i = 0; i < hst.size(); i++) status[i] = hst[i];
    if (bad_layout) return fail(h, GRAAL_E_STATE, "graal_close_rings: corrupt layout (contig labels, positions or lengths do not agree)");
    for (size_t i = 0; i < hst.size(); i++)
        if (hst[i] != GRAAL_RINGEDIT_OK) return fail(h, GRAAL_E_ARG, "graal_close_rings: a contig cannot be closed (see status)");
    return layout_replaced(h, h->cur);   // (written in place, in the current buffer)
}

} // extern "C"
