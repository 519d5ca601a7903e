// layout_slots.h -- the slot numbering of a layout, built once for every whole-layout scorer: junctions.h, rings.h and maps.h hold a
// LayoutSlots in their buffers, links.h's LayoutRecs holds one for links, insertions, span moves and excisions.  Included by
// graal_hip.hip after score_common.h (it uses Ctx, SoaPtr, CK, blocks_for and score_common.h's STEP_CK, and dev_buf.h's DevBuf).
//
// Number the fragments of the layout by slots: contigs by ascending label, a contig's fragments consecutive, in position order (contig
// label -> member count -> exclusive scan -> offset + position).  The numbering is built from the layout fields, not taken from the
// engine's position index: a scorer does not relabel, and so leaves the ranked layout, the carried total and a pending commit's correction
// exactly as they were.  edit.h keeps its own count and slot kernels: its label range (2n + 4) and its at[] claim differ.
#pragma once

namespace {

// cnt: members per contig label; base: a label's first slot (the exclusive scan of cnt over the n + 3 labels); slot: per fragment, -1 for
// one without; err[0]: the flags of a corrupt layout (bit 0 a label, bit 1 a position or slot out of range; the callers OR their own bits),
// err[1]: rings.h's longest contig; tmp: hipCUB's scratch for the scan, and for the owner's own scans when it asked for more.
// The owners' rule (dev_buf.h) holds for this set and for every set built on it: n stays 0 until the whole set is allocated.
struct LayoutSlots {
    int n = 0;
    DevBuf<int> cnt, base, slot;
    DevBuf<unsigned> err;
    DevBuf<void> tmp;
};

// Sized to the engine's n, reallocated when it changes or when the owner needs more scratch than there is.
int slots_reserve(Ctx* h, LayoutSlots& L, size_t own_tmp_bytes = 0)
{
    const int n = h->n;
    if (L.n == n && L.tmp.count >= own_tmp_bytes) return GRAAL_OK;
    size_t tb = 0;
    CK(hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (int*)nullptr, (int*)nullptr, n + 3, h->stream));
    CK(group_realloc(L.n, n, L.cnt, n + 3, L.base, n + 3, L.slot, n, L.err, 2, L.tmp, std::max(tb, own_tmp_bytes)));
    return GRAAL_OK;
}

// members per contig label (labels lie in [0, n + 2]: the mutations keep them in [0, n_contigs + 2])
__global__ void k_jn_count(SoaPtr s, int n, int* __restrict__ cnt, unsigned* __restrict__ err)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= n) return;
    const int c = s.p[F_IDC][f];
    if (c < 0 || c > n + 2) { atomicOr(err, 1u); return; }
    atomicAdd(&cnt[c], 1);
}

// The opening of the prep kernels (k_jn_prep, k_rg_prep, k_ln_prep): fragment f's slot, written to slot_of[f]; -1, with error bit 2 set,
// when its label, its position or the slot itself is out of range.
__device__ __forceinline__ int slot_claim(SoaPtr s, int n, int f, const int* __restrict__ cnt, const int* __restrict__ base,
                                          int* __restrict__ slot_of, unsigned* __restrict__ err)
{
    const int c = s.p[F_IDC][f], pos = s.p[F_POS][f];
    int slot = -1;
    if (c >= 0 && c <= n + 2 && pos >= 0 && pos < cnt[c]) slot = base[c] + pos;
    if (slot < 0 || slot >= n) { atomicOr(err, 2u); slot = -1; }
    slot_of[f] = slot;
    return slot;
}

// Clears the flags and the counts, counts the members per label and scans them, on the engine's stream; the owner's prep kernel follows.
int slots_count(Ctx* h, LayoutSlots& L)
{
    const int n = L.n;
    hipStream_t s = h->stream;
    int rc = GRAAL_OK;
    do {
        STEP_CK(hipMemsetAsync(L.err, 0, sizeof(unsigned) * 2, s));
        STEP_CK(hipMemsetAsync(L.cnt, 0, sizeof(int) * (size_t)(n + 3), s));
        k_jn_count<<<blocks_for(n, 256), 256, 0, s>>>(h->soa[h->cur], n, L.cnt, L.err);
        STEP_CK(hipGetLastError());
        size_t tb = L.tmp.count;
        STEP_CK(hipcub::DeviceScan::ExclusiveSum(L.tmp.p, tb, L.cnt.p, L.base.p, n + 3, s));
    } while (false);
    return rc;
}

// The flags, read back behind everything launched so far: the caller leaves when they are set (a corrupt layout: the slots are not to be
// trusted, nothing reads them).  A step of its own, so that a caller's kernels can add their bits first.
int slots_read_err(Ctx* h, const LayoutSlots& L, unsigned& flags, unsigned* longest_contig = nullptr)
{
    unsigned w[2] = {0, 0};
    int rc = GRAAL_OK;
    do {
        STEP_CK(hipMemcpyAsync(w, L.err, sizeof(unsigned) * (longest_contig ? 2 : 1), hipMemcpyDeviceToHost, h->stream));
        STEP_CK(hipStreamSynchronize(h->stream));
    } while (false);
    flags = w[0];
    if (longest_contig) *longest_contig = w[1];
    return rc;
}

} // namespace
