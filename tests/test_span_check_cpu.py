"""span_check.h through libgraal_hostcheck's hc_span_check: what graal_block_flips / graal_block_swaps decide on the host about a
caller's spans -- the first offending span and the reason, or every span's status byte and the order of the scored records -- against a
plain restatement (a pairwise overlap test against every earlier span instead of the ordered set), for both calls' descriptors.

The layout: two linear contigs of 12 and 5 fragments and a ring of 6, slots in that order; fragment 23 has no slot.  The rows are what
k_sp_gather writes: all slots and labels -1 when one of the span's fragments has no slot; for a call without a mid, mid = last."""
import ctypes

import numpy as np
import pytest

from graal_amd.lib import FLIP_CIRCULAR, FLIP_VALID, FLIP_WHOLE, SWAP_CIRCULAR, SWAP_VALID
from tests import util

NO_SLOT, TWO_CONTIGS, MID_BEFORE_FIRST, LAST_NOT_BEHIND_MID, OVERLAP = 1, 2, 3, 4, 5
KINDS = {                                        # kind -> (hc_span_check's number, has a mid, whole-contig status or None, valid, circular)
    "flips": (0, False, FLIP_WHOLE, FLIP_VALID, FLIP_CIRCULAR),
    "swaps": (1, True, None, SWAP_VALID, SWAP_CIRCULAR),
}
REASONS = {"flips": (NO_SLOT, TWO_CONTIGS, MID_BEFORE_FIRST, OVERLAP),
           "swaps": (NO_SLOT, TWO_CONTIGS, MID_BEFORE_FIRST, LAST_NOT_BEHIND_MID, OVERLAP)}
N_LISTS = 3000

CONTIGS = ((0, 12, 0), (12, 5, 0), (17, 6, 1))   # (first slot, fragments, ring)
N_SLOTS = 23
_rs = np.random.RandomState(7)
FRAG_OF_SLOT = _rs.permutation(N_SLOTS)          # fragment ids 0 .. 22 in slot order; fragment 23 has no slot
SLOT_OF = np.append(np.argsort(FRAG_OF_SLOT), -1)
LAB_OF_SLOT = np.concatenate([[c] * n for c, (_, n, _) in enumerate(CONTIGS)])
LEN_OF_SLOT = _rs.randint(500, 4000, N_SLOTS)
START_OF_SLOT = np.concatenate([np.cumsum(LEN_OF_SLOT[a:a + n]) - LEN_OF_SLOT[a:a + n] for a, n, _ in CONTIGS])


def gathered(first, mid, last):
    """k_sp_gather's row for the span of fragments (first, mid, last)."""
    sf, sm, sl = (int(SLOT_OF[f]) for f in (first, mid, last))
    if min(sf, sm, sl) < 0:
        return [-1] * 6 + [0] * 6
    a, n, ring = CONTIGS[LAB_OF_SLOT[sf]]
    return [sf, sm, sl, LAB_OF_SLOT[sf], LAB_OF_SLOT[sm], LAB_OF_SLOT[sl], START_OF_SLOT[sf], START_OF_SLOT[sm] + LEN_OF_SLOT[sm],
            START_OF_SLOT[sl] + LEN_OF_SLOT[sl], a, n, ring]


def random_list(rs, has_mid):
    """1 to 8 spans: mostly short well-formed ones inside a random contig, now and then three fragments drawn from all 24."""
    rows = []
    for _ in range(rs.randint(1, 9)):
        if rs.rand() < 0.12:
            f, m, l = (int(x) for x in rs.randint(0, N_SLOTS + 1, 3))
            if not has_mid:
                m = l
        else:
            a, n, _ = CONTIGS[rs.randint(0, 3)]
            length = min(n, rs.randint(2 if has_mid else 1, 6))
            p0 = rs.randint(0, n - length + 1)
            pm = p0 + rs.randint(0, length - 1) if has_mid else p0 + length - 1
            f, m, l = (int(FRAG_OF_SLOT[a + p]) for p in (p0, pm, p0 + length - 1))
        rows.append(gathered(f, m, l))
    return np.array(rows, dtype=np.int32)


def restated(rows, kind):
    """(first offender, reason), or (None, status bytes, the caller's indices of the scored spans by first slot)."""
    _, has_mid, whole, valid, circular = KINDS[kind]
    for k, (sf, sm, sl, lf, lm, ll) in enumerate(rows[:, :6].tolist()):
        if sf < 0:
            return k, NO_SLOT
        if lf != lm or lf != ll:
            return k, TWO_CONTIGS
        if sf > sm:
            return k, MID_BEFORE_FIRST
        if has_mid and sm >= sl:
            return k, LAST_NOT_BEHIND_MID
        if any(not (sl < f2 or l2 < sf) for f2, l2 in rows[:k, [0, 2]].tolist()):
            return k, OVERLAP
    st, scored = [], []
    for k, r in enumerate(rows.tolist()):
        if r[11]:
            st.append(circular)
        elif whole is not None and r[0] == r[9] and r[2] == r[9] + r[10] - 1:
            st.append(whole)
        else:
            st.append(valid)
            scored.append(k)
    return None, st, sorted(scored, key=lambda k: rows[k, 0])


def lists(kind):
    rs = np.random.RandomState(20 + KINDS[kind][0])
    return [random_list(rs, KINDS[kind][1]) for _ in range(N_LISTS)]


def counts(kind, results):
    refused = [r[1] for r in results if r[0] is not None]
    accepted = [r for r in results if r[0] is None]
    return {why: refused.count(why) for why in REASONS[kind]}, sum(len(r[2]) >= 2 for r in accepted), [b for r in accepted for b in r[1]]


@pytest.mark.parametrize("kind", ["flips", "swaps"])
def test_the_seeds_cover_every_reason_and_enough_accepted_lists(kind):
    by_reason, accepted2, st = counts(kind, [restated(rows, kind) for rows in lists(kind)])
    assert min(by_reason.values()) >= 20, by_reason
    assert accepted2 >= 100
    _, _, whole, valid, circular = KINDS[kind]
    assert st.count(valid) >= 100 and st.count(circular) >= 20 and (whole is None or st.count(whole) >= 20)


@pytest.mark.parametrize("kind", ["flips", "swaps"])
def test_span_check_equals_the_restatement(kind):
    L = util.hostcheck()
    L.hc_span_check.restype = ctypes.c_int
    i32p, u8p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_uint8)
    L.hc_span_check.argtypes = [ctypes.c_int, ctypes.c_int, i32p, i32p, u8p, i32p]
    results = []
    for rows in lists(kind):
        nb = len(rows)
        out, st, ids = np.full(2, -7, np.int32), np.full(nb, 255, np.uint8), np.full(nb, -7, np.int32)
        m = L.hc_span_check(KINDS[kind][0], nb, rows.ctypes.data_as(i32p), out.ctypes.data_as(i32p), st.ctypes.data_as(u8p),
                            ids.ctypes.data_as(i32p))
        want = restated(rows, kind)
        results.append(want)
        if want[0] is not None:
            assert m == -1 and (int(out[0]), int(out[1])) == want, rows
        else:
            assert m == len(want[2]) and int(out[0]) == -1 and int(out[1]) == 0, rows
            assert st.tolist() == want[1] and ids[:m].tolist() == want[2], rows
    by_reason, accepted2, _ = counts(kind, results)
    assert min(by_reason.values()) >= 20 and accepted2 >= 100
