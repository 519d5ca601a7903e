// span_check.h -- what the host decides about a caller's spans before graal_block_flips / graal_block_swaps (span_moves.h) or
// graal_block_excisions (excise.h) score them:
// the first span the call is refused for, or every span's status and the scored spans sorted by first slot.  Pure arithmetic on the rows
// k_sp_gather wrote: no HIP calls, no handle, no side effects.  Shared with host_check.cpp, so that the CPU tests pin every refusal and
// the order of the records without a device (tests/test_span_check_cpu.py).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../include/graal_hip.h"

// per span of the caller, from its fragments first, mid and last (a call without a mid: mid = last): their slots (-1: a fragment without
// one) and contigs, the bp interval [s0, e1) with the breakpoint sm behind mid, its contig's slots
struct SpanInfo { int slot_f, slot_m, slot_l, lab_f, lab_m, lab_l, s0, sm, e1, cfirst, ccnt, circ; };
// the scored spans, sorted by first slot; id: the caller's index
struct SpanRec { int s0, sm, e1, first, mid, last, cfirst, clast, id, pad; };

// the two calls: the same move with different data
struct SpanKind {
    const char* fn;                                  // the function's name and the spans' noun, for messages
    const char* noun;
    bool has_mid;                                    // the caller names a breakpoint (else mid = last: the run Y behind it is empty)
    int rev;                                         // the run X is reversed inside its new interval
    int whole;                                       // the status of a span that is its whole contig, set aside unscored; -1: scored
    unsigned char valid, circular, nonfinite;
};
constexpr SpanKind SPAN_FLIPS = {"graal_block_flips", "block", false, 1, GRAAL_FLIP_WHOLE, GRAAL_FLIP_VALID, GRAAL_FLIP_CIRCULAR, GRAAL_FLIP_NONFINITE};
constexpr SpanKind SPAN_SWAPS = {"graal_block_swaps", "swap", true, 0, -1, GRAAL_SWAP_VALID, GRAAL_SWAP_CIRCULAR, GRAAL_SWAP_NONFINITE};
// (graal_block_excisions, excise.h: the span is cut out of its contig; the spans are checked and ordered the same way)
constexpr SpanKind SPAN_EXCISE = {"graal_block_excisions", "span", false, 0, GRAAL_EXCISE_WHOLE, GRAAL_EXCISE_VALID, GRAAL_EXCISE_CIRCULAR,
                                  GRAAL_EXCISE_NONFINITE};

// why a call is refused, in the order the checks are made on a span
enum SpanReason { SPAN_OK = 0, SPAN_NO_SLOT, SPAN_TWO_CONTIGS, SPAN_MID_BEFORE_FIRST, SPAN_LAST_NOT_BEHIND_MID, SPAN_OVERLAP };

struct SpanChecked {
    int off = -1;                                    // the first offending span by the caller's numbering (-1: none) and why
    SpanReason why = SPAN_OK;
    std::vector<unsigned char> st;                   // else: every span's status, and the scored ones
    std::vector<SpanRec> rec;
};

inline SpanChecked span_check(const SpanInfo* info, int nb, const SpanKind& K)
{
    SpanChecked out;
    // (overlap: the spans enter an ordered set in the caller's order; those already in it are pairwise disjoint, so the first span
    // that meets one of its two neighbours there is the first that overlaps an earlier span)
    std::map<int, int> by_first;                     // first slot -> last slot
    for (int k = 0; k < nb && out.off < 0; k++) {
        const SpanInfo& I = info[k];
        SpanReason why = SPAN_OK;
        if (I.slot_f < 0) why = SPAN_NO_SLOT;
        else if (I.lab_f != I.lab_m || I.lab_f != I.lab_l) why = SPAN_TWO_CONTIGS;
        else if (I.slot_f > I.slot_m) why = SPAN_MID_BEFORE_FIRST;
        else if (K.has_mid && I.slot_m >= I.slot_l) why = SPAN_LAST_NOT_BEHIND_MID;
        else {
            auto nx = by_first.lower_bound(I.slot_f);    // the first span that starts at or behind this one
            bool hit = nx != by_first.end() && nx->first <= I.slot_l;
            if (!hit && nx != by_first.begin()) hit = std::prev(nx)->second >= I.slot_f;
            if (hit) why = SPAN_OVERLAP;
            else by_first.emplace(I.slot_f, I.slot_l);
        }
        if (why != SPAN_OK) { out.off = k; out.why = why; }
    }
    if (out.off >= 0) return out;
    std::vector<int> order((size_t)nb);
    for (int k = 0; k < nb; k++) order[(size_t)k] = k;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return info[a].slot_f < info[b].slot_f; });
    out.st.resize((size_t)nb);
    for (int i = 0; i < nb; i++) {
        const int k = order[(size_t)i];
        const SpanInfo& I = info[k];
        if (I.circ) { out.st[(size_t)k] = K.circular; continue; }
        if (K.whole >= 0 && I.slot_f == I.cfirst && I.slot_l == I.cfirst + I.ccnt - 1) { out.st[(size_t)k] = (unsigned char)K.whole; continue; }
        out.st[(size_t)k] = K.valid;
        out.rec.push_back(SpanRec{I.s0, I.sm, I.e1, I.slot_f, I.slot_m, I.slot_l, I.cfirst, I.cfirst + I.ccnt - 1, k, 0});
    }
    return out;
}

// the refusal's reason in the call's words
inline void span_reason_text(const SpanKind& K, SpanReason why, char* buf, size_t len)
{
    switch (why) {
    case SPAN_NO_SLOT: snprintf(buf, len, "a fragment without a slot"); break;
    case SPAN_TWO_CONTIGS: snprintf(buf, len, "%s lie on two contigs", K.has_mid ? "first, mid and last" : "first and last"); break;
    case SPAN_MID_BEFORE_FIRST: snprintf(buf, len, "%s lies before first", K.has_mid ? "mid" : "last"); break;
    case SPAN_LAST_NOT_BEHIND_MID: snprintf(buf, len, "last does not lie behind mid"); break;
    case SPAN_OVERLAP: snprintf(buf, len, "overlaps an earlier %s", K.noun); break;
    default: snprintf(buf, len, "nothing"); break;
    }
}
