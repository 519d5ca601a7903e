// links_boot.h -- bootstrap support for every listed link between contig ends, all replicates in one call (graal_end_links_bootstrap).
// Included by graal_hip.hip after links.h (it uses LnBuf, ln_links, the contact unit ln_contact / ln_comb / ln_comb_term, ln_find,
// k_lb_init, wave_runs.h's run_head / run_tail / run_sum and simulate.h's SimStream and sim_poisson).
//
// Poisson bootstrap of read pairs, as junction_boot.h: in replicate r contact k counts
//   ob*_{k,r} = sim_poisson(ob_k, SimStream(row_k, col_k, 2 | r << 8, seed))
// -- the junction bootstrap's stream, tag and sampler: under one seed replicate r of both calls is the same resampled dataset.
// L*_r(link) is what graal_end_links returns for the link with every count replaced by ob*_{k,r} (contacts that drew 0 stay, with count
// 0).  Only what multiplies a count changes:
//   L*_r = M + C_r + sum over the contigs the link reverses of mirc_r[contig],
//   C_r    = the link's record terms to_q(ob* . (ln ex_joined - ln ex_trans)), less the mirror's contact term where the link prices the
//            pair itself (ln_comb_term), each rounded to Q once per (contact, end combination, replicate);
//   mirc_r = the contact part of mirror[C] (ln_mirror_term), rounded to Q once per (contact, replicate);
//   M      = L - qc - sum of the data's mirc over the reversed contigs: the mass (k_ln_mass), the quirk's pairs (k_ln_quirk) and the mass
//            part of mirror[C] (k_ln_mirror), computed once.  qc is the table's word before the mass is added, the data's mirc what the
//            insert pass left in mirror[C] before k_ln_mirror (ln_links keeps a copy): int64 sums, so the split is exact.
// Every sum is int64: a replicate is a function of (layout, tables, parameters, contacts, seed, r) alone, bit-identical from call to
// call, for any grid, any n_rep and any batching.
//
// Kernels, on the engine's stream, behind graal_end_links' own (ln_links):
//   k_lkb_prep -- per link: M, and the link's index at its table slot (the slot -> link map; other slots hold -1);
//   k_lkb_nnz  -- per batch of RB replicates: the row-sorted list, 64 consecutive contacts per wave.  Per contact, once: the 4 keys, their
//                 units, the link at each key's slot (find-only probe: a replicate record whose key the data's table does not hold, or
//                 holds unlisted, is dropped) and the run heads / tails of equal links along the wave.  A wave without a record or a
//                 mirror term moves on without drawing.  Per replicate: one draw per lane, shared by the 4 combinations; a segmented sum
//                 per combination and one for the mirror, one 64-bit atomic per run tail into C[r * m + link] / mirc[r * (n + 3) + C];
//   k_lkb_best -- per (replicate, link): L*_r in place of C, atomicMax of it at its two ends; k_lkb_arg: atomicMin of the partner among
//                 the links that reach the end's maximum (k_lb_out / k_lb_arg's scheme, on RB x 2n arrays);
//   k_lkb_fold -- one thread per link walks the batch's replicates in order, no atomics: support, sum, min, max, mutual;
//   k_lkb_finish -- the call's status (a replicate term that did not fit Q marks the link non-finite) and zeros where it is not valid.
// Batches: RB = the largest count <= 64 whose per-replicate arrays (C, mirc, per-end best Q and partner) fit LKB_BATCH_BYTES, at least 1.
#pragma once

namespace {

constexpr int LKB_MAX_REP = 1024;
constexpr unsigned long long LKB_BATCH_BYTES = 256ull << 20;

__global__ void k_lkb_prep(long long m, const int* __restrict__ vs, const int* __restrict__ ea, const int* __restrict__ eb,
                           const int* __restrict__ lab, const long long* __restrict__ q, const long long* __restrict__ tq,
                           const long long* __restrict__ mirc, int mq, long long* __restrict__ fix, int* __restrict__ s2l)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    const int i = vs[k];
    s2l[i] = (int)k;
    long long v = q[k] - tq[i];
    if (mq) {
        if ((ea[k] & 1) == 0) v -= mirc[lab[ea[k] >> 1]];
        if ((eb[k] & 1) == 1) v -= mirc[lab[eb[k] >> 1]];
    }
    fix[k] = v;
}

// Every shuffle below (run_head, run_tail, run_sum) is executed by all 64 lanes: the branches around them are wave-uniform (ballots).
__global__ __launch_bounds__(256) void k_lkb_nnz(const int* __restrict__ row, const int* __restrict__ col, const int* __restrict__ cnt, long long nnz,
                                                 const LnSub* __restrict__ sub, const Stat* __restrict__ stat, const LnCtg* __restrict__ ctg,
                                                 float nfpb, Par par, int quirk, unsigned long long cap,
                                                 const unsigned long long* __restrict__ keys, const int* __restrict__ s2l,
                                                 unsigned long long seed, int r0, int rb, long long m, int nl, long long* __restrict__ C,
                                                 int* __restrict__ lbad, long long* __restrict__ mirc, int* __restrict__ mcbad)
{
    const int lane = threadIdx.x & 63;
    const long long wave = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long long n_waves = ((long long)gridDim.x * blockDim.x) >> 6;
    for (long long k0 = wave * 64; k0 < nnz; k0 += n_waves * 64) {   // (wave-uniform bounds: the run sums need the whole wave)
        const long long k = k0 + lane;
        LnSub X = {-1, -1, 0, 0, 0, 0, 0, 0}, Y = X;
        unsigned ra = 0, cb = 0;
        if (k < nnz) { ra = (unsigned)row[k]; cb = (unsigned)col[k]; X = sub[ra]; Y = sub[cb]; }
        LnContact U;
        ln_contact(X, Y, quirk, nfpb, par, U);
        if (__ballot(U.pair || U.m_on) == 0ull) continue;
        const double ob = k < nnz ? (double)__int_as_float(cnt[k]) : 0.0;
        // ---- once per contact: the link, the unit and the flags of each end combination
        int link[4] = {-1, -1, -1, -1};
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        bool sub_m[4] = {false, false, false, false};
        if (U.pair) {
            const LnCtg CX = ctg[X.label], CY = ctg[Y.label];
            const Stat SX = stat[X.frag], SY = stat[Y.frag];
            const double ln_et = ln_contact_trans(U, nfpb, par);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                LnComb G;
                ln_comb(U, X, Y, CX, CY, SX, SY, c, ln_et, nfpb, par, G);
                if (!G.has_t && !G.sub_m) continue;                  // (no term multiplies the count: nothing to re-form)
                const long long i = ln_find(keys, cap, G.key);
                if (i >= 0) link[c] = s2l[i];
                t[c] = G.t; sub_m[c] = G.sub_m;
            }
        }
        const int mlab = U.m_on ? U.mlabel : -1;
        const bool any = link[0] >= 0 || link[1] >= 0 || link[2] >= 0 || link[3] >= 0;
        if (__ballot(any || mlab >= 0) == 0ull) continue;
        int head[4];
        bool tail[4], live[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            live[c] = __ballot(link[c] >= 0) != 0ull;
            head[c] = 0; tail[c] = false;
            if (live[c]) { head[c] = run_head(link[c]); tail[c] = run_tail(link[c]); }
        }
        const bool m_live = __ballot(mlab >= 0) != 0ull;
        int m_head = 0;
        bool m_tail = false;
        if (m_live) { m_head = run_head(mlab); m_tail = run_tail(mlab); }
        // ---- per replicate: one draw, the terms, a segmented sum per combination and one atomic per run
        for (int r = 0; r < rb; r++) {
            double obr = 0.0;
            if (any || mlab >= 0) {
                SimStream st(ra, cb, 2u | ((unsigned)(r0 + r) << 8), seed);
                obr = (double)sim_poisson(ob, st);
            }
            long long m_term;
            bool m_bad;
            ln_mirror_term(U, obr, m_term, m_bad);
            if (m_live) {
                if (m_bad && mlab >= 0) atomicOr(&mcbad[mlab], 1);
                if (__ballot(m_term != 0) != 0ull) {
                    const long long v = run_sum(mlab >= 0 ? m_term : 0, m_head);
                    if (m_tail && mlab >= 0 && v != 0)
                        atomicAdd((unsigned long long*)&mirc[(size_t)r * (size_t)nl + mlab], (unsigned long long)v);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if (!live[c]) continue;
                long long q = 0;
                bool bad = false;
                if (link[c] >= 0) {
                    LnComb G;
                    G.t = t[c]; G.has_t = true; G.sub_m = sub_m[c]; G.in_win = false; G.key = 0;
                    ln_comb_term(G, obr, m_term, m_bad, q, bad);     // (has_t with t = 0: to_q(0) = 0, as no term)
                    if (bad) { atomicOr(&lbad[link[c]], 1); q = 0; }
                }
                if (__ballot(q != 0) == 0ull) continue;
                const long long v = run_sum(q, head[c]);
                if (tail[c] && link[c] >= 0 && v != 0)
                    atomicAdd((unsigned long long*)&C[(size_t)r * (size_t)m + link[c]], (unsigned long long)v);
            }
        }
    }
}

// the contact parts of the mirrors of the contigs a link reverses, in replicate row `mr`
__device__ __forceinline__ long long lkb_mirrors(int e_a, int e_b, const int* __restrict__ lab, const long long* __restrict__ mr)
{
    long long v = 0;
    if ((e_a & 1) == 0) v += mr[lab[e_a >> 1]];
    if ((e_b & 1) == 1) v += mr[lab[e_b >> 1]];
    return v;
}

// per (replicate of the batch, link): L*_r in place of the contact sum (0 where the data's link has no score), and the highest per end
__global__ void k_lkb_best(long long m, int rb, const int* __restrict__ ea, const int* __restrict__ eb, const int* __restrict__ lab,
                           const unsigned char* __restrict__ st, const long long* __restrict__ fix, int mq, int nl, long long n2,
                           long long* __restrict__ C, const long long* __restrict__ mirc, long long* __restrict__ bq)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * rb) return;
    const long long r = idx / m, k = idx - r * m;
    if (st[k] != GRAAL_LINK_VALID) { C[idx] = 0; return; }
    long long v = fix[k] + C[idx];
    if (mq) v += lkb_mirrors(ea[k], eb[k], lab, mirc + (size_t)r * (size_t)nl);
    C[idx] = v;
    atomicMax(&bq[r * n2 + ea[k]], v);
    atomicMax(&bq[r * n2 + eb[k]], v);
}

// the lowest partner among the valid links that reach an end's highest L*_r
__global__ void k_lkb_arg(long long m, int rb, const int* __restrict__ ea, const int* __restrict__ eb, const unsigned char* __restrict__ st,
                          long long n2, const long long* __restrict__ C, const long long* __restrict__ bq, int* __restrict__ be)
{
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= m * rb) return;
    const long long r = idx / m, k = idx - r * m;
    if (st[k] != GRAAL_LINK_VALID) return;
    const long long v = C[idx];
    if (v == bq[r * n2 + ea[k]]) atomicMin(&be[r * n2 + ea[k]], eb[k]);
    if (v == bq[r * n2 + eb[k]]) atomicMin(&be[r * n2 + eb[k]], ea[k]);
}

// One thread per link walks the batch's replicates in order.  first: this batch begins the call (the statistics start here).
__global__ __launch_bounds__(256) void k_lkb_fold(long long m, int rb, int first, long long threshold, const int* __restrict__ ea,
                                                  const int* __restrict__ eb, const unsigned char* __restrict__ st, long long n2,
                                                  const long long* __restrict__ C, const int* __restrict__ be, int* __restrict__ sup,
                                                  int* __restrict__ mut, long long* __restrict__ sum, long long* __restrict__ mn,
                                                  long long* __restrict__ mx)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    int s = 0, u = 0;
    long long a = 0, lo = 0, hi = 0;
    if (!first) { s = sup[k]; u = mut[k]; a = sum[k]; lo = mn[k]; hi = mx[k]; }
    if (st[k] == GRAAL_LINK_VALID) {
        const int e_a = ea[k], e_b = eb[k];
        for (int r = 0; r < rb; r++) {
            const long long v = C[(size_t)r * (size_t)m + k];
            const bool over = v > threshold;
            s += over ? 1 : 0;
            a += v;
            lo = (first && r == 0) ? v : min(lo, v);
            hi = (first && r == 0) ? v : max(hi, v);
            u += (over && be[r * n2 + e_a] == e_b && be[r * n2 + e_b] == e_a) ? 1 : 0;
        }
    }
    sup[k] = s; mut[k] = u; sum[k] = a; mn[k] = lo; mx[k] = hi;
}

// the call's status: the data's, or non-finite where a replicate term of the link or of a mirror it adds did not fit Q; zeros there
__global__ void k_lkb_finish(long long m, const int* __restrict__ ea, const int* __restrict__ eb, const int* __restrict__ lab,
                             const unsigned char* __restrict__ st, const int* __restrict__ lbad, const int* __restrict__ mcbad, int mq,
                             unsigned char* __restrict__ out, int* __restrict__ sup, int* __restrict__ mut, long long* __restrict__ sum,
                             long long* __restrict__ mn, long long* __restrict__ mx)
{
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= m) return;
    int b = st[k] != GRAAL_LINK_VALID || lbad[k];
    if (mq && (ea[k] & 1) == 0) b |= mcbad[lab[ea[k] >> 1]];
    if (mq && (eb[k] & 1) == 1) b |= mcbad[lab[eb[k] >> 1]];
    out[k] = b ? GRAAL_LINK_NONFINITE : GRAAL_LINK_VALID;
    if (b) { sup[k] = 0; mut[k] = 0; sum[k] = 0; mn[k] = 0; mx[k] = 0; }
}

} // namespace

extern "C" {

int graal_end_links_bootstrap(graal_ctx* h, int32_t min_frags, uint64_t seed, int32_t n_rep, int64_t threshold_q, int32_t want_rep,
                              int64_t* n_links)
{
    if (!h || !n_links) return GRAAL_E_ARG;
    if (min_frags < 1) return fail(h, GRAAL_E_ARG, "graal_end_links_bootstrap: min_frags must be >= 1");
    if (n_rep < 1 || n_rep > LKB_MAX_REP) return fail(h, GRAAL_E_ARG, "graal_end_links_bootstrap: n_rep must be in 1 .. 1024");
    if (const int rc = score_entry(h, "graal_end_links_bootstrap")) return rc;
    *n_links = 0;
    if (!h->ln) h->ln = new LnBuf();
    LnBuf* Lb = h->ln;
    Lb->n_links = -1;
    Lb->boot_links = -1;
    Lb->boot_rep = n_rep; Lb->boot_want = want_rep != 0;
    std::vector<long long>().swap(Lb->k_rep);                        // (the last call's matrix leaves the host here)
    if (h->n < 1) { Lb->n_links = 0; Lb->boot_links = 0; return GRAAL_OK; }
    const int n = h->n, nl = n + 3;
    const long long n2 = 2ll * n;
    hipStream_t s = h->stream;
    LayoutRecs& R = Lb->R;
    CandTable& T = Lb->T;
    const int quirk = (h->mode & GRAAL_MODE_REF_TRANS_ACCU) ? 1 : 0;
    const int mq = quirk && h->n_ubins > 0;
    LnCount C;
    long long m = 0;
    const char* why = nullptr;
    char msg[320];
    unsigned long long need = 0;
    int rc = GRAAL_OK;
    do {
        STEP_CK(Lb->kc_mir.reserve_grow((size_t)nl));
        STEP_CK(Lb->kc_bad.reserve_grow((size_t)nl));
        if ((rc = ln_links(h, Lb, min_frags, "graal_end_links_bootstrap", Lb->kc_mir, C, m, why, msg, sizeof msg, need)) || why || C.err) break;
        if (m == 0) break;
        Lb->n_links = m;                                             // (the table is graal_end_links': its fetch may follow)
        // device memory on top of the link table's: the slot -> link map, the per-label and per-link arrays, and a batch of RB replicates
        const unsigned long long per_rep = 8ull * (unsigned long long)m + 8ull * (unsigned long long)nl + (8ull + 4ull) * (unsigned long long)n2;
        const int RB = (int)std::max<unsigned long long>(1, std::min<unsigned long long>(std::min(64, (int)n_rep), LKB_BATCH_BYTES / per_rep));
        need += 4ull * C.cap + 12ull * (unsigned long long)nl + (unsigned long long)m * (8 * 4 + 4 * 3 + 1) + (unsigned long long)RB * per_rep;
        if (need > (unsigned long long)GRAAL_LINKS_MAX_BYTES || (unsigned long long)m * (unsigned long long)RB > (unsigned long long)INT_MAX * 256ull) {
            snprintf(msg, sizeof msg, "graal_end_links_bootstrap: %lld links in batches of %d replicates need %llu bytes, over the budget of %llu "
                     "bytes (GRAAL_LINKS_MAX_BYTES): use a larger min_frags", m, RB, need, (unsigned long long)GRAAL_LINKS_MAX_BYTES);
            why = msg;
            break;
        }
        STEP_CK(Lb->k_s2l.reserve_grow((size_t)C.cap));
        STEP_CK(group_grow(Lb->kcap, (size_t)m, Lb->k_fix, m, Lb->k_sum, m, Lb->k_mn, m, Lb->k_mx, m, Lb->k_sup, m, Lb->k_mut, m, Lb->k_lbad, m,
                           Lb->k_st, m));
        STEP_CK(Lb->kb_c.reserve_grow((size_t)RB * (size_t)m));
        STEP_CK(Lb->kb_mir.reserve_grow((size_t)RB * (size_t)nl));
        STEP_CK(Lb->kb_bq.reserve_grow((size_t)RB * (size_t)n2));
        STEP_CK(Lb->kb_be.reserve_grow((size_t)RB * (size_t)n2));
        if (want_rep) {                                              // (host memory, outside the device budget: refused, not thrown)
            const unsigned long long rep_bytes = 8ull * (unsigned long long)n_rep * (unsigned long long)m;
            bool have = rep_bytes <= (unsigned long long)GRAAL_LINKS_MAX_BYTES;      // (the device budget bounds the host matrix too)
            try {
                if (have) Lb->k_rep.assign((size_t)n_rep * (size_t)m, 0);
            } catch (const std::exception&) {
                have = false;
            }
            if (!have) {
                std::vector<long long>().swap(Lb->k_rep);
                snprintf(msg, sizeof msg, "graal_end_links_bootstrap: the replicate matrix of %d x %lld links needs %llu bytes of host memory "
                         "(at most GRAAL_LINKS_MAX_BYTES, %llu, are kept): call without want_rep, or with fewer replicates", (int)n_rep, m,
                         rep_bytes, (unsigned long long)GRAAL_LINKS_MAX_BYTES);
                why = msg;
                break;
            }
        }
        STEP_CK(hipMemsetAsync(Lb->k_s2l, 0xff, sizeof(int) * (size_t)C.cap, s));
        STEP_CK(hipMemsetAsync(Lb->k_lbad, 0, sizeof(int) * (size_t)m, s));
        STEP_CK(hipMemsetAsync(Lb->kc_bad, 0, sizeof(int) * (size_t)nl, s));
        k_lkb_prep<<<blocks_for(m, 256), 256, 0, s>>>(m, Lb->vs, Lb->ea, Lb->eb, R.lab, Lb->q, T.tq, Lb->kc_mir, mq, Lb->k_fix, Lb->k_s2l);
        STEP_CK(hipGetLastError());
        for (int r0 = 0; r0 < n_rep && !rc; r0 += RB) {
            const int rb = std::min(RB, (int)n_rep - r0);
            const long long cells = (long long)rb * m;
            STEP_CK(hipMemsetAsync(Lb->kb_c, 0, sizeof(long long) * (size_t)cells, s));
            STEP_CK(hipMemsetAsync(Lb->kb_mir, 0, sizeof(long long) * (size_t)rb * (size_t)nl, s));
            if (h->nnz > 0) {
                k_lkb_nnz<<<stream_blocks(h->nnz), 256, 0, s>>>(h->row, h->col, h->cnt, h->nnz, R.sub, h->stat_frag, R.ctg, h->nfpb, h->par, quirk,
                                                                C.cap, T.keys, Lb->k_s2l, (unsigned long long)seed, r0, rb, m, nl, Lb->kb_c,
                                                                Lb->k_lbad, Lb->kb_mir, Lb->kc_bad);
                STEP_CK(hipGetLastError());
            }
            k_lb_init<<<blocks_for((long long)rb * n2, 256), 256, 0, s>>>((long long)rb * n2, Lb->kb_bq, Lb->kb_be);
            k_lkb_best<<<blocks_for(cells, 256), 256, 0, s>>>(m, rb, Lb->ea, Lb->eb, R.lab, Lb->st, Lb->k_fix, mq, nl, n2, Lb->kb_c, Lb->kb_mir,
                                                              Lb->kb_bq);
            k_lkb_arg<<<blocks_for(cells, 256), 256, 0, s>>>(m, rb, Lb->ea, Lb->eb, Lb->st, n2, Lb->kb_c, Lb->kb_bq, Lb->kb_be);
            k_lkb_fold<<<blocks_for(m, 256), 256, 0, s>>>(m, rb, r0 == 0 ? 1 : 0, (long long)threshold_q, Lb->ea, Lb->eb, Lb->st, n2, Lb->kb_c,
                                                          Lb->kb_be, Lb->k_sup, Lb->k_mut, Lb->k_sum, Lb->k_mn, Lb->k_mx);
            STEP_CK(hipGetLastError());
            if (want_rep) {                                          // (the next batch clears the rows: they leave first)
                STEP_CK(hipMemcpyAsync(Lb->k_rep.data() + (size_t)r0 * (size_t)m, Lb->kb_c, sizeof(long long) * (size_t)cells,
                                       hipMemcpyDeviceToHost, s));
                STEP_CK(hipStreamSynchronize(s));
            }
        }
        if (rc) break;
        k_lkb_finish<<<blocks_for(m, 256), 256, 0, s>>>(m, Lb->ea, Lb->eb, R.lab, Lb->st, Lb->k_lbad, Lb->kc_bad, mq, Lb->k_st, Lb->k_sup,
                                                        Lb->k_mut, Lb->k_sum, Lb->k_mn, Lb->k_mx);
        STEP_CK(hipGetLastError());
        STEP_CK(hipStreamSynchronize(s));
    } while (false);
    if (const int r = score_exit(h, "graal_end_links_bootstrap", rc, why, C.err)) { Lb->n_links = -1; return r; }
    Lb->n_links = m;
    Lb->boot_links = m;
    *n_links = m;
    return GRAAL_OK;
}

int graal_end_links_bootstrap_fetch(graal_ctx* h, int32_t* end_a, int32_t* end_b, int64_t* q, int64_t* contacts, uint8_t* status,
                                    int32_t* support, int32_t* mutual, int64_t* q_sum, int64_t* q_min, int64_t* q_max, int64_t* q_rep,
                                    int64_t cap)
{
    if (!h || !end_a || !end_b || !q || !contacts || !status || !support || !mutual || !q_sum || !q_min || !q_max) return GRAAL_E_ARG;
    LnBuf* Lb = h->ln;
    if (!Lb || Lb->boot_links < 0) return fail(h, GRAAL_E_STATE, "graal_end_links_bootstrap_fetch: call graal_end_links_bootstrap first");
    if (q_rep && !Lb->boot_want) return fail(h, GRAAL_E_ARG, "graal_end_links_bootstrap_fetch: q_rep needs a call with want_rep set");
    const long long m = Lb->boot_links;
    if (cap < m) return fail(h, GRAAL_E_ARG, "graal_end_links_bootstrap_fetch: cap is smaller than the number of links");
    if (m == 0) return GRAAL_OK;
    CK(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    CK(hipMemcpyAsync(end_a, Lb->ea, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(end_b, Lb->eb, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(q, Lb->q, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(contacts, Lb->c, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(status, Lb->k_st, (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(support, Lb->k_sup, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(mutual, Lb->k_mut, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(q_sum, Lb->k_sum, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(q_min, Lb->k_mn, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(q_max, Lb->k_mx, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (q_rep) memcpy(q_rep, Lb->k_rep.data(), sizeof(long long) * (size_t)Lb->boot_rep * (size_t)m);
    for (long long k = 0; k < m; k++) {
        if (status[k] == GRAAL_LINK_VALID) continue;
        q[k] = 0;
        if (q_rep) for (int r = 0; r < Lb->boot_rep; r++) q_rep[(size_t)r * (size_t)m + k] = 0;
    }
    return GRAAL_OK;
}

} // extern "C"
