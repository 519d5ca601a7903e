// edit.h -- a batch of cuts and joins applied to the layout in one call (graal_edit_layout).
// Included by graal_hip.hip after excise.h (it uses Ctx, SoaPtr, the F_* field indices, fail, wait_own, dev_buf.h's DevBuf and score_common.h's
// layout_replaced).
//
// The rules are those of include/graal_hip.h (graal_edit_layout); tests/edit_reference.py restates them in numpy.  Kernels, all on the
// engine's stream:
//   k_ed_count / exclusive scan / k_ed_slot -- slots: contig label -> count -> offset + position (labels < 2n + 4, as graal_upload_frags
//                 accepts them), the fragment of every slot, the largest label;
//   k_ed_cuts, k_ed_cut_dup -- validate the cuts, count them per fragment and per contig (and the last cut position of a ring);
//   k_ed_mark, an inclusive max scan, k_ed_piece, k_ed_fresh, exclusive scan, k_ed_piece_lab -- the pieces the cuts leave: each slot
//                 starts a piece or not, the scan gives every fragment its piece's head; the head holds the piece's fragment count, bp
//                 length, tail, circular flag and label (fresh labels ranked by head fragment);
//   k_ed_joins, k_ed_join_dup -- validate the joins on the pieces; every joined end learns its partner end;
//   k_ed_jinit, k_ed_jump x R, k_ed_cycle -- chain ranking by pointer jumping over piece ends.  Entering piece P at end x, the walk leaves
//                 it through the other end m(x) and enters the next piece at the partner of m(x): nxt(x).  Each end carries the sums of
//                 the pieces from its own on (pieces, fragments, bp), the smallest joined exit end and the smallest label; R rounds with
//                 2^R > joins + 1 end every path, and an end whose pointer is still set lies on a cycle;
//   k_ed_write -- one thread per fragment writes its 14 fields into the other layout buffer.
#pragma once

namespace {

struct EdAgg { int np, nf, nbp, minx, minlab, term, nxt, pad; };   // a walk's sums from an end on (np pieces, nf fragments, nbp bp)

struct EdBuf {
    int n = 0;
    DevBuf<int> cnt, base, ncut, lastcut;                            // per label (2n + 5)
    DevBuf<int> slot, at, cutc, mark, hs, ph, pp, pob, pcnt, plbp, ptail, plab, fresh, frank;   // per fragment
    DevBuf<int> ejc, ejo;                                            // per end (2n)
    DevBuf<EdAgg> agg[2];
    DevBuf<int> scal;                                                // [0] max label, [1] error flags
    DevBuf<void> tmp;
    DevBuf<int> d_cut, d_ea, d_eb, d_st; int ccap = 0, jcap = 0;
};

void ed_free(EdBuf* b) { delete b; }

struct EdMax { __device__ __forceinline__ int operator()(int a, int b) const { return a > b ? a : b; } };

__global__ void k_ed_count(SoaPtr s, int n, int* __restrict__ cnt, int* __restrict__ scal)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int c = s.p[F_IDC][f];
    if (c < 0 || c >= 2 * n + 4) { atomicOr(&scal[1], 1); return; }
    atomicAdd(&cnt[c], 1);
    atomicMax(&scal[0], c);
}

__global__ void k_ed_slot(SoaPtr s, int n, const int* __restrict__ cnt, const int* __restrict__ base, int* __restrict__ slot,
                          int* __restrict__ at, int* __restrict__ scal)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int c = s.p[F_IDC][f], pos = s.p[F_POS][f];
    if (c < 0 || c >= 2 * n + 4 || pos < 0 || pos >= cnt[c]) { atomicOr(&scal[1], 2); slot[f] = -1; return; }
    const int sl = base[c] + pos;
    slot[f] = sl;
    if (atomicCAS(&at[sl], -1, f) != -1) atomicOr(&scal[1], 4);    // (two fragments at one position)
}

__global__ void k_ed_cuts(SoaPtr s, int n, int n_cuts, const int* __restrict__ cut, const int* __restrict__ cnt, int* __restrict__ cutc,
                          int* __restrict__ ncut, int* __restrict__ lastcut, int* __restrict__ st)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cuts) return;
    const int f = cut[i];
    if (f < 0 || f >= n) { st[i] = GRAAL_EDIT_BAD_CUT; return; }
    const int c = s.p[F_IDC][f], pos = s.p[F_POS][f], ring = s.p[F_CIRC][f] == 1;
    if (ring ? cnt[c] < 2 : pos >= cnt[c] - 1) { st[i] = GRAAL_EDIT_BAD_CUT; return; }
    atomicAdd(&cutc[f], 1);
    atomicAdd(&ncut[c], 1);
    if (ring) atomicMax(&lastcut[c], pos);
}

__global__ void k_ed_cut_dup(int n_cuts, const int* __restrict__ cut, const int* __restrict__ cutc, int* __restrict__ st)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_cuts && st[i] == GRAAL_EDIT_OK && cutc[cut[i]] > 1) st[i] = GRAAL_EDIT_DUP_CUT;
}

// mark[s] = s when slot s starts a piece, -1 otherwise: position 0 of a linear contig or of an uncut ring, and the slot after a cut
// (a ring's position 0 follows its last position)
__global__ void k_ed_mark(SoaPtr s, int n, const int* __restrict__ at, const int* __restrict__ cutc, const int* __restrict__ cnt,
                          const int* __restrict__ ncut, int* __restrict__ mark)
{
    const int sl = blockIdx.x * blockDim.x + threadIdx.x;
    if (sl >= n) return;
    const int f = at[sl];
    const int c = s.p[F_IDC][f], pos = s.p[F_POS][f];
    const bool ring = s.p[F_CIRC][f] == 1;
    bool m;
    if (pos > 0) m = cutc[at[sl - 1]] > 0;
    else if (!ring || ncut[c] == 0) m = true;
    else m = cutc[at[sl + cnt[c] - 1]] > 0;
    mark[sl] = m ? sl : -1;
}

// every fragment's piece: head, position in the piece, bp offset in the piece
__global__ void k_ed_piece(SoaPtr s, int n, const int* __restrict__ at, const int* __restrict__ slot, const int* __restrict__ hs,
                           const int* __restrict__ base, const int* __restrict__ cnt, const int* __restrict__ lastcut, int* __restrict__ ph,
                           int* __restrict__ pp, int* __restrict__ pob, int* __restrict__ pcnt, int* __restrict__ plbp)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int c = s.p[F_IDC][f], pos = s.p[F_POS][f], sl = slot[f];
    int h = hs[sl];
    if (h < base[c]) h = base[c] + (lastcut[c] + 1) % cnt[c];        // (a ring's piece that wraps past its last position)
    const int hf = at[h], hpos = s.p[F_POS][hf];
    ph[f] = hf;
    pp[f] = pos >= hpos ? pos - hpos : pos + cnt[c] - hpos;
    pob[f] = pos >= hpos ? s.p[F_START][f] - s.p[F_START][hf] : s.p[F_START][f] + s.p[F_LCONTBP][f] - s.p[F_START][hf];
    atomicAdd(&pcnt[hf], 1);
    atomicAdd(&plbp[hf], s.p[F_LEN][f]);
}

// heads: a fresh label unless the piece holds its contig's position 0
__global__ void k_ed_fresh(SoaPtr s, int n, const int* __restrict__ at, const int* __restrict__ base, const int* __restrict__ ph,
                           int* __restrict__ fresh)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    fresh[f] = (ph[f] == f && ph[at[base[s.p[F_IDC][f]]]] != f) ? 1 : 0;
}

__global__ void k_ed_piece_lab(SoaPtr s, int n, const int* __restrict__ ph, const int* __restrict__ pp, const int* __restrict__ pcnt,
                               const int* __restrict__ fresh, const int* __restrict__ frank, const int* __restrict__ scal,
                               int* __restrict__ ptail, int* __restrict__ plab)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int hf = ph[f];
    if (pp[f] == pcnt[hf] - 1) ptail[hf] = f;
    if (hf == f) plab[f] = fresh[f] ? scal[0] + 1 + frank[f] : s.p[F_IDC][f];
}

__device__ __forceinline__ bool ed_uncut_ring(SoaPtr s, int f, const int* __restrict__ ncut)
{
    return s.p[F_CIRC][f] == 1 && ncut[s.p[F_IDC][f]] == 0;
}

// the end status of e after the cuts: OK, BAD_END (out of range / not a piece end) or CIRCULAR
__device__ __forceinline__ int ed_end_ok(SoaPtr s, int n, int e, const int* __restrict__ ph, const int* __restrict__ pp,
                                         const int* __restrict__ pcnt, const int* __restrict__ ncut)
{
    if (e < 0 || e >= 2 * n) return GRAAL_EDIT_BAD_END;
    const int f = e >> 1;
    if (ed_uncut_ring(s, f, ncut)) return GRAAL_EDIT_CIRCULAR;
    const bool is_end = (e & 1) ? pp[f] == pcnt[ph[f]] - 1 : pp[f] == 0;
    return is_end ? GRAAL_EDIT_OK : GRAAL_EDIT_BAD_END;
}

__global__ void k_ed_joins(SoaPtr s, int n, int n_joins, const int* __restrict__ ea, const int* __restrict__ eb, const int* __restrict__ ph,
                           const int* __restrict__ pp, const int* __restrict__ pcnt, const int* __restrict__ ncut, int* __restrict__ ejc,
                           int* __restrict__ ejo, int* __restrict__ st)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_joins) return;
    const int a = ea[j], b = eb[j];
    int r = ed_end_ok(s, n, a, ph, pp, pcnt, ncut);
    const int rb = ed_end_ok(s, n, b, ph, pp, pcnt, ncut);
    if (r == GRAAL_EDIT_OK) r = rb;
    if (r == GRAAL_EDIT_OK && ph[a >> 1] == ph[b >> 1]) r = GRAAL_EDIT_SAME_CONTIG;
    st[j] = r;
    if (r != GRAAL_EDIT_OK) return;
    atomicAdd(&ejc[a], 1); atomicAdd(&ejc[b], 1);
    ejo[a] = b; ejo[b] = a;                                          // (an end used twice is refused below: which write wins does not matter)
}

__global__ void k_ed_join_dup(int n_joins, const int* __restrict__ ea, const int* __restrict__ eb, const int* __restrict__ ejc, int* __restrict__ st)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_joins && st[j] == GRAAL_EDIT_OK && (ejc[ea[j]] > 1 || ejc[eb[j]] > 1)) st[j] = GRAAL_EDIT_END_TWICE;
}

// the other end of the piece of end x
__device__ __forceinline__ int ed_mate(int x, const int* __restrict__ ph, const int* __restrict__ ptail)
{
    return (x & 1) ? 2 * ph[x >> 1] : 2 * ptail[x >> 1] + 1;
}

__device__ __forceinline__ bool ed_piece_end(int x, const int* __restrict__ ph, const int* __restrict__ ptail)
{
    const int f = x >> 1;
    return (x & 1) ? ptail[ph[f]] == f : ph[f] == f;
}

__global__ void k_ed_jinit(int n, const int* __restrict__ ph, const int* __restrict__ ptail, const int* __restrict__ pcnt,
                           const int* __restrict__ plbp, const int* __restrict__ plab, const int* __restrict__ ejc, const int* __restrict__ ejo,
                           EdAgg* __restrict__ agg)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= 2 * n) return;
    EdAgg a = {0, 0, 0, INT_MAX, INT_MAX, x, -1, 0};
    if (ed_piece_end(x, ph, ptail)) {
        const int m = ed_mate(x, ph, ptail), hf = ph[x >> 1];
        a.np = 1; a.nf = pcnt[hf]; a.nbp = plbp[hf]; a.minlab = plab[hf];
        if (ejc[m] > 0) { a.minx = m; a.nxt = ejo[m]; }
    }
    agg[x] = a;
}

__global__ void k_ed_jump(int n, const EdAgg* __restrict__ in, EdAgg* __restrict__ out)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= 2 * n) return;
    EdAgg a = in[x];
    if (a.nxt >= 0) {
        const EdAgg b = in[a.nxt];
        a.np += b.np; a.nf += b.nf; a.nbp += b.nbp;
        a.minx = min(a.minx, b.minx); a.minlab = min(a.minlab, b.minlab);
        a.term = b.term; a.nxt = b.nxt;
    }
    out[x] = a;
}

__global__ void k_ed_cycle(int n_joins, const int* __restrict__ ea, const EdAgg* __restrict__ agg, int* __restrict__ st, int* __restrict__ scal)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n_joins && agg[ea[j]].nxt >= 0) { st[j] = GRAAL_EDIT_CYCLE; atomicOr(&scal[1], 8); }
}

__global__ void k_ed_write(SoaPtr s, SoaPtr o, int n, const int* __restrict__ base, const int* __restrict__ at, const int* __restrict__ cnt,
                           const int* __restrict__ ncut, const int* __restrict__ ph, const int* __restrict__ pp, const int* __restrict__ pob,
                           const int* __restrict__ pcnt, const int* __restrict__ plbp, const int* __restrict__ ptail,
                           const int* __restrict__ plab, const int* __restrict__ ejc, const int* __restrict__ ejo, const EdAgg* __restrict__ agg)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    for (int k = 0; k < GRAAL_N_FIELDS; k++) o.p[k][f] = s.p[k][f];
    const int c = s.p[F_IDC][f], pos = s.p[F_POS][f], hf = ph[f], tf = ptail[hf];
    const int eh = 2 * hf, et = 2 * tf + 1;
    const bool joined = ejc[eh] > 0 || ejc[et] > 0;
    if (!joined && ncut[c] == 0) return;                             // (an untouched contig keeps every field)
    const int k = pp[f], cn = cnt[c], b = base[c];
    // the fragments before / after f in its piece (the slot order, a ring's last position followed by its first)
    const int up = k == 0 ? -1 : at[b + (pos + cn - 1) % cn];
    const int dn = k == pcnt[hf] - 1 ? -1 : at[b + (pos + 1) % cn];
    int npos = k, nstart = pob[f], ori = s.p[F_ORI][f], prv = up, nxt = dn, lc = pcnt[hf], lbp = plbp[hf], lab = plab[hf];
    if (joined) {
        // the canonical direction enters the piece at z: the direction whose joined exit ends hold the chain's smallest joined end
        const EdAgg ah = agg[eh], at_ = agg[et];
        const int start_h = ed_mate(at_.term, ph, ptail), start_t = ed_mate(ah.term, ph, ptail);   // where the walks through eh / et start
        const EdAgg th = agg[start_h], tt = agg[start_t];
        const bool via_h = th.minx < tt.minx;
        const int z = via_h ? eh : et;
        const EdAgg az = via_h ? ah : at_, tot = via_h ? th : tt;
        const bool rev = !via_h;
        const int foff = tot.nf - az.nf, boff = tot.nbp - az.nbp;
        npos = foff + (rev ? lc - 1 - k : k);
        nstart = boff + (rev ? lbp - pob[f] - s.p[F_LEN][f] : pob[f]);
        if (rev) ori = -ori;
        const int zm = via_h ? et : eh;                              // the exit end
        const int before = ejc[z] > 0 ? (ejo[z] >> 1) : -1, after = ejc[zm] > 0 ? (ejo[zm] >> 1) : -1;
        prv = rev ? dn : up; nxt = rev ? up : dn;
        if (prv < 0) prv = before;
        if (nxt < 0) nxt = after;
        lc = tot.nf; lbp = tot.nbp; lab = tot.minlab;
    }
    o.p[F_POS][f] = npos; o.p[F_IDC][f] = lab; o.p[F_START][f] = nstart; o.p[F_CIRC][f] = 0; o.p[F_PREV][f] = prv; o.p[F_NEXT][f] = nxt;
    o.p[F_LCONT][f] = lc; o.p[F_LCONTBP][f] = lbp; o.p[F_ORI][f] = ori;
}

} // namespace

extern "C" {

int graal_edit_layout(graal_ctx* h, int32_t n_cuts, const int32_t* cut_after, int32_t n_joins, const int32_t* end_a, const int32_t* end_b,
                      int32_t* status)
{
    if (!h || n_cuts < 0 || n_joins < 0 || (n_cuts > 0 && !cut_after) || (n_joins > 0 && (!end_a || !end_b)) || (n_cuts + n_joins > 0 && !status))
        return GRAAL_E_ARG;
    if (!h->have_frags) return fail(h, GRAAL_E_STATE, "graal_edit_layout: upload the fragments first");
    if (h->has_rep) return fail(h, GRAAL_E_UNSUPPORTED, "graal_edit_layout: bins with several copies (graal_upload_repeats) are not supported");
    if (h->x_host || h->nccl_comm) return fail(h, GRAAL_E_STATE, "graal_edit_layout: one rank only (an exchange or RCCL is attached)");
    for (int i = 0; i < n_cuts + n_joins; i++) status[i] = GRAAL_EDIT_OK;
    if (n_cuts + n_joins == 0) return GRAAL_OK;
    CK(hipSetDevice(h->device));
    // (what graal_upload_frags waits for: graal_begin_step's relabel kernels, the last commit's own-pixel correction)
    CK(hipStreamSynchronize(h->stream));
    if (h->fstream) CK(hipStreamSynchronize(h->fstream));
    if (h->own_pending) { const int rc = wait_own(h, nullptr, nullptr); if (rc) return rc; }
    const int n = h->n, NL = 2 * n + 5;
    hipStream_t s = h->stream;
    if (!h->ed) h->ed = new EdBuf();
    EdBuf* E = h->ed;
    if (E->n != n) {
        size_t b1 = 0, b2 = 0, b3 = 0;
        CK(hipcub::DeviceScan::ExclusiveSum(nullptr, b1, (int*)nullptr, (int*)nullptr, NL, s));
        CK(hipcub::DeviceScan::InclusiveScan(nullptr, b2, (int*)nullptr, (int*)nullptr, EdMax(), n, s));
        CK(hipcub::DeviceScan::ExclusiveSum(nullptr, b3, (int*)nullptr, (int*)nullptr, n, s));
        const size_t n2 = 2 * (size_t)n;
        CK(group_realloc(E->n, n, E->cnt, NL, E->base, NL, E->ncut, NL, E->lastcut, NL, E->slot, n, E->at, n, E->cutc, n, E->mark, n, E->hs, n,
                         E->ph, n, E->pp, n, E->pob, n, E->pcnt, n, E->plbp, n, E->ptail, n, E->plab, n, E->fresh, n, E->frank, n, E->ejc, n2,
                         E->ejo, n2, E->agg[0], n2, E->agg[1], n2, E->scal, 4, E->tmp, std::max(b1, std::max(b2, b3))));
    }
    if (n_cuts > E->ccap || n_joins > E->jcap) {
        const int cc = std::max(n_cuts, 1), jc = std::max(n_joins, 1);
        E->jcap = 0;
        CK(group_realloc(E->ccap, cc, E->d_cut, cc, E->d_ea, jc, E->d_eb, jc, E->d_st, cc + jc));
        E->jcap = jc;
    }
    int* st_cut = E->d_st;
    int* st_join = E->d_st + n_cuts;
    if (n_cuts) CK(hipMemcpyAsync(E->d_cut, cut_after, sizeof(int) * (size_t)n_cuts, hipMemcpyHostToDevice, s));
    if (n_joins) {
        CK(hipMemcpyAsync(E->d_ea, end_a, sizeof(int) * (size_t)n_joins, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(E->d_eb, end_b, sizeof(int) * (size_t)n_joins, hipMemcpyHostToDevice, s));
    }
    CK(hipMemsetAsync(E->d_st, 0, sizeof(int) * (size_t)(n_cuts + n_joins), s));
    CK(hipMemsetAsync(E->scal, 0, sizeof(int) * 4, s));
    CK(hipMemsetAsync(E->cnt, 0, sizeof(int) * (size_t)NL, s));
    CK(hipMemsetAsync(E->ncut, 0, sizeof(int) * (size_t)NL, s));
    CK(hipMemsetAsync(E->lastcut, 0xff, sizeof(int) * (size_t)NL, s));
    CK(hipMemsetAsync(E->at, 0xff, sizeof(int) * (size_t)n, s));
    CK(hipMemsetAsync(E->cutc, 0, sizeof(int) * (size_t)n, s));
    CK(hipMemsetAsync(E->pcnt, 0, sizeof(int) * (size_t)n, s));
    CK(hipMemsetAsync(E->plbp, 0, sizeof(int) * (size_t)n, s));
    CK(hipMemsetAsync(E->ejc, 0, sizeof(int) * 2 * (size_t)n, s));
    const SoaPtr sp = h->soa[h->cur];
    const int nb = blocks_for(n, 256);
    int scal[4] = {0, 0, 0, 0};
    // ---- slots; a corrupt layout stops here, before anything indexes by label or slot
    k_ed_count<<<nb, 256, 0, s>>>(sp, n, E->cnt, E->scal);
    CK(hipGetLastError());
    size_t tb = E->tmp.count;
    CK(hipcub::DeviceScan::ExclusiveSum(E->tmp.p, tb, E->cnt.p, E->base.p, NL, s));
    k_ed_slot<<<nb, 256, 0, s>>>(sp, n, E->cnt, E->base, E->slot, E->at, E->scal);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(scal, E->scal, sizeof scal, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (scal[1]) {
        char msg[160];
        snprintf(msg, sizeof msg, "graal_edit_layout: corrupt layout (contig labels or positions out of range, flags %d)", scal[1]);
        return fail(h, GRAAL_E_STATE, msg);
    }
    // ---- cuts and pieces
    if (n_cuts) {
        k_ed_cuts<<<blocks_for(n_cuts, 256), 256, 0, s>>>(sp, n, n_cuts, E->d_cut, E->cnt, E->cutc, E->ncut, E->lastcut, st_cut);
        k_ed_cut_dup<<<blocks_for(n_cuts, 256), 256, 0, s>>>(n_cuts, E->d_cut, E->cutc, st_cut);
        CK(hipGetLastError());
    }
    k_ed_mark<<<nb, 256, 0, s>>>(sp, n, E->at, E->cutc, E->cnt, E->ncut, E->mark);
    CK(hipGetLastError());
    tb = E->tmp.count;
    CK(hipcub::DeviceScan::InclusiveScan(E->tmp.p, tb, E->mark.p, E->hs.p, EdMax(), n, s));
    k_ed_piece<<<nb, 256, 0, s>>>(sp, n, E->at, E->slot, E->hs, E->base, E->cnt, E->lastcut, E->ph, E->pp, E->pob, E->pcnt, E->plbp);
    k_ed_fresh<<<nb, 256, 0, s>>>(sp, n, E->at, E->base, E->ph, E->fresh);
    CK(hipGetLastError());
    tb = E->tmp.count;
    CK(hipcub::DeviceScan::ExclusiveSum(E->tmp.p, tb, E->fresh.p, E->frank.p, n, s));
    k_ed_piece_lab<<<nb, 256, 0, s>>>(sp, n, E->ph, E->pp, E->pcnt, E->fresh, E->frank, E->scal, E->ptail, E->plab);
    CK(hipGetLastError());
    // ---- joins
    if (n_joins) {
        k_ed_joins<<<blocks_for(n_joins, 256), 256, 0, s>>>(sp, n, n_joins, E->d_ea, E->d_eb, E->ph, E->pp, E->pcnt, E->ncut, E->ejc, E->ejo, st_join);
        k_ed_join_dup<<<blocks_for(n_joins, 256), 256, 0, s>>>(n_joins, E->d_ea, E->d_eb, E->ejc, st_join);
        CK(hipGetLastError());
    }
    std::vector<int> hst((size_t)(n_cuts + n_joins));
    int n_fresh[2] = {0, 0};
    CK(hipMemcpyAsync(hst.data(), E->d_st, sizeof(int) * hst.size(), hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&n_fresh[0], E->frank + (n - 1), sizeof(int), hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&n_fresh[1], E->fresh + (n - 1), sizeof(int), hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(scal, E->scal, sizeof scal, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    for (size_t i = 0; i < hst.size(); i++) status[i] = hst[i];
    for (size_t i = 0; i < hst.size(); i++)
        if (hst[i] != GRAAL_EDIT_OK) return fail(h, GRAAL_E_ARG, "graal_edit_layout: a cut or a join is not valid (see status)");
    if ((long long)scal[0] + n_fresh[0] + n_fresh[1] >= 2ll * n + 4)
        return fail(h, GRAAL_E_ARG, "graal_edit_layout: the new contig labels would reach 2n+4: relabel the layout first");
    // ---- chains: pointer jumping over piece ends
    int cur = 0;
    k_ed_jinit<<<blocks_for(2ll * n, 256), 256, 0, s>>>(n, E->ph, E->ptail, E->pcnt, E->plbp, E->plab, E->ejc, E->ejo, E->agg[0]);
    CK(hipGetLastError());
    if (n_joins) {
        int rounds = 0;
        while ((1ll << rounds) <= (long long)n_joins + 1) rounds++;   // 2^rounds > the longest path (joins + 1 pieces)
        for (int r = 0; r < rounds; r++) {
            k_ed_jump<<<blocks_for(2ll * n, 256), 256, 0, s>>>(n, E->agg[cur], E->agg[1 - cur]);
            cur = 1 - cur;
        }
        k_ed_cycle<<<blocks_for(n_joins, 256), 256, 0, s>>>(n_joins, E->d_ea, E->agg[cur], st_join, E->scal);
        CK(hipGetLastError());
        CK(hipMemcpyAsync(scal, E->scal, sizeof scal, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        if (scal[1] & 8) {
            CK(hipMemcpy(hst.data() + n_cuts, st_join, sizeof(int) * (size_t)n_joins, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < hst.size(); i++) status[i] = hst[i];
            return fail(h, GRAAL_E_ARG, "graal_edit_layout: the joins close a cycle of contigs (see status)");
        }
    }
    // ---- the fields, into the other layout buffer; the result ends in buffer 0, as after graal_upload_frags
    const int out = 1 - h->cur;
    k_ed_write<<<nb, 256, 0, s>>>(sp, h->soa[out], n, E->base, E->at, E->cnt, E->ncut, E->ph, E->pp, E->pob, E->pcnt, E->plbp, E->ptail, E->plab,
                                  E->ejc, E->ejo, E->agg[cur]);
    CK(hipGetLastError());
    return layout_replaced(h, out);
}

} // extern "C"
