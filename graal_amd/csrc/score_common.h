// score_common.h -- what the whole-layout scorers and commits (junctions.h, rings.h, links.h, insert.h, span_moves.h, excise.h, edit.h,
// maps.h) share on the host side: the entry refusals and the common exits, the step check of their do { ... } while (false) frames, the
// two launch sizes they all compute, the tail of a commit that rewrote the layout, and the
// open-addressing candidate table.
// Included by graal_hip.hip before layout_slots.h and junctions.h (it uses Ctx, fail, CK, refresh and sync_args).
#pragma once

namespace {

// One step of a scorer's `do { ... } while (false)` frame: a HIP error is recorded in h->err, `rc` becomes GRAAL_E_HIP and the frame is left
// (the caller drains the stream and returns rc).  Needs `h` and an `int rc` in scope.
#define STEP_CK(call) { const hipError_t e_ = (call); if (e_ != hipSuccess) { h->err = hipGetErrorString(e_); rc = GRAAL_E_HIP; break; } }

// What every whole-layout call `fn` refuses before it touches the device.  missing: what the call needs uploaded and does not find (null:
// nothing is missing); the scorers and graal_close_rings differ in that alone.
int layout_refusal(Ctx* h, const char* fn, const char* missing)
{
    const char* why = missing;
    int code = GRAAL_E_STATE;
    if (!why && h->has_rep) { why = "bins with several copies (graal_upload_repeats) are not supported"; code = GRAAL_E_UNSUPPORTED; }
    if (!why && (h->x_host || h->nccl_comm)) why = "one rank only (an exchange or RCCL is attached)";
    if (why) return fail(h, code, (std::string(fn) + ": " + why).c_str());
    return GRAAL_OK;
}

// The scorers' entry: they need everything uploaded; then the device is selected.
int score_entry(Ctx* h, const char* fn)
{
    const bool have = h->have_sub && h->have_par && h->have_frags && h->have_contacts;
    if (const int rc = layout_refusal(h, fn, have ? nullptr : "upload sub-fragments, parameters, fragments and contacts first")) return rc;
    CK(hipSetDevice(h->device));
    return GRAAL_OK;
}

// How a scorer's frame ends: a HIP error (the stream is drained first), a refusal `why`, the flags `err` of a corrupt layout, or GRAAL_OK.
int score_exit(Ctx* h, const char* fn, int rc, const char* why, unsigned err)
{
    if (rc) { (void)hipStreamSynchronize(h->stream); return rc; }
    if (why) return fail(h, GRAAL_E_UNSUPPORTED, why);
    if (!err) return GRAAL_OK;
    char msg[200];
    snprintf(msg, sizeof msg, "%s: corrupt layout (contig labels or positions out of range, flags %u)", fn, err);
    return fail(h, GRAAL_E_STATE, msg);
}

// Blocks of 256 threads for a kernel that streams the contact list 64 consecutive contacts per wave: four waves' worth of contacts per
// block, at most 2048 blocks (the waves stride over the rest), at least one.
inline int stream_blocks(long long nnz)
{
    const long long waves = (nnz + 63) / 64;
    return (int)std::max<long long>(1, std::min<long long>((waves + 3) / 4, 2048));
}

// Waves per tile of 64 slots in k_full_mass_t's tiling (k_jn_mass, k_rg_mass, k_mp_cis): one per 8 chunks of 64 slots of the longest
// contig, at most 16.
inline int mass_stripes(int longest_contig) { return std::min(16, std::max(1, ((longest_contig + 63) / 64 + 7) / 8)); }

// The tail of a commit that rewrote the layout in buffer `from_buffer` (graal_edit_layout, graal_close_rings): the result ends in buffer 0
// and the engine in graal_upload_frags' state (the stat_frag table is unchanged: no fragment changes its bin).
int layout_replaced(Ctx* h, int from_buffer)
{
    hipStream_t s = h->stream;
    if (from_buffer != 0)
        CK(hipMemcpyAsync(h->soa_mem[0], h->soa_mem[from_buffer], sizeof(int) * (size_t)h->n * GRAAL_N_FIELDS, hipMemcpyDeviceToDevice, s));
    CK(hipStreamSynchronize(s));
    h->cur = 0; h->ranks_valid = false; h->pending_commits = 0; h->begin_launched = false; h->stats_from_apply = false;
    h->order_valid = false;
    h->carry_q = 0; h->carry_bad = true;
    if (const int rc = refresh(h)) return rc;
    CK(hipStreamSynchronize(s));
    return sync_args(h);
}

// The candidate table: open addressing keyed by a 64-bit key (ln_slot), per slot a Q sum, a contact count, flags and the selection byte of
// DeviceSelect::Flagged; and the hipCUB scratch of the passes behind it.  Both grow to the largest size a call needed.
struct CandTable {
    DevBuf<unsigned long long> keys; DevBuf<long long> tq, tc; DevBuf<int> tf; DevBuf<unsigned char> tsel; size_t cap = 0;
    DevBuf<void> stmp;
};
constexpr unsigned long long TABLE_SLOT_BYTES = 8 + 8 + 8 + 4 + 1;   // key, q, contacts, flags, selection byte

// slots for an upper bound of the distinct keys (load factor <= 2/3)
inline unsigned long long table_cap(unsigned long long bound) { return bound + bound / 2 + 64; }

hipError_t table_reserve(CandTable& T, unsigned long long cap)
{
    return group_grow(T.cap, cap, T.keys, cap, T.tq, cap, T.tc, cap, T.tf, cap, T.tsel, cap);
}

hipError_t scratch_reserve(CandTable& T, size_t bytes) { return T.stmp.reserve_grow(bytes); }

// (the table is used at size `cap`, whatever its allocation: the probe sequence depends on it)
hipError_t table_clear(CandTable& T, unsigned long long cap, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(T.keys, 0xff, sizeof(unsigned long long) * cap, s);
    if (e == hipSuccess) e = hipMemsetAsync(T.tq, 0, sizeof(long long) * cap, s);
    if (e == hipSuccess) e = hipMemsetAsync(T.tc, 0, sizeof(long long) * cap, s);
    if (e == hipSuccess) e = hipMemsetAsync(T.tf, 0, sizeof(int) * cap, s);
    return e;
}

} // namespace
