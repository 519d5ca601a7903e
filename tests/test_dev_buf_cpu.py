"""dev_buf.h through libgraal_hostcheck's hc_devbuf_*: the owner of a device array and the group form, over a counting host allocator
(host_check.cpp) that keeps the set of live blocks, fails on the k-th allocation when told to, and reports a free of a block that is
not live.  That set is the whole leak and double-free check.

What is held to: the exact policy reallocates when the wanted count differs and the grow-only policy when it exceeds what is held; a
buffer is freed BEFORE its replacement is allocated (the peak of live blocks never exceeds the members); a group whose k-th allocation
fails reports the failure, reads size 0, holds only null or live pointers, and the next reserve frees each survivor exactly once; a
moved-from owner frees nothing; pinned words come back zeroed.  An element count of 0 releases the buffer and holds a null pointer
without calling the allocator: what hipMalloc of 0 bytes gave the call sites before."""
import ctypes

import numpy as np
import pytest

from tests import util

EXACT, GROW, REALLOC = 0, 1, 2
MOVE = 2
NULL, LIVE, DANGLING = 0, 1, 2
MEMBERS = 5
_i64p = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture
def hc():
    L = util.hostcheck()
    L.hc_devbuf_arm.argtypes = [ctypes.c_int64]
    L.hc_devbuf_arm.restype = None
    L.hc_devbuf_stats.argtypes = [_i64p]
    L.hc_devbuf_stats.restype = None
    L.hc_devbuf_one.argtypes = [ctypes.c_int, ctypes.c_int64, _i64p]
    L.hc_devbuf_group.argtypes = [ctypes.c_int, ctypes.c_int64, _i64p, _i64p]
    L.hc_devbuf_pinned_zeroed.argtypes = [ctypes.c_int]
    L.hc_devbuf_destroy.restype = None
    L.hc_devbuf_destroy()
    L.hc_devbuf_arm(0)
    assert stats(L)["live"] == 0
    yield L
    L.hc_devbuf_destroy()


def stats(L):
    out = np.zeros(5, np.int64)
    L.hc_devbuf_stats(out.ctypes.data_as(_i64p))
    return dict(zip(("allocs", "frees", "bad", "live", "peak"), (int(x) for x in out)))


def one(L, what, n=0):
    """(error, count held, pointer state, the allocator's counters for this call alone)"""
    L.hc_devbuf_arm(0)
    out = np.zeros(2, np.int64)
    e = L.hc_devbuf_one(what, n, out.ctypes.data_as(_i64p))
    return e, int(out[0]), int(out[1]), stats(L)


def group(L, what, want, counts, fail_at=0):
    """(error, size field, the five pointer states, the allocator's counters for this call alone)"""
    L.hc_devbuf_arm(fail_at)
    c = np.asarray(counts, np.int64)
    out = np.zeros(1 + MEMBERS, np.int64)
    e = L.hc_devbuf_group(what, want, c.ctypes.data_as(_i64p), out.ctypes.data_as(_i64p))
    return e, int(out[0]), [int(x) for x in out[1:]], stats(L)


def destroyed_clean(L):
    L.hc_devbuf_arm(0)
    L.hc_devbuf_destroy()
    s = stats(L)
    assert s["live"] == 0 and s["bad"] == 0, s
    return s


def test_exact_policy(hc):
    e, count, state, s = one(hc, EXACT, 100)
    assert (e, count, state) == (0, 100, LIVE) and (s["allocs"], s["frees"]) == (1, 0)
    e, count, state, s = one(hc, EXACT, 100)                 # the same count: no allocator call
    assert (e, count, state) == (0, 100, LIVE) and (s["allocs"], s["frees"]) == (0, 0)
    for n in (40, 400):                                      # smaller, larger: one free, then one allocation
        e, count, state, s = one(hc, EXACT, n)
        assert (e, count, state) == (0, n, LIVE) and (s["allocs"], s["frees"], s["bad"]) == (1, 1, 0)
        assert s["peak"] == 1                                # the free came first: old and new never live together
    assert destroyed_clean(hc)["frees"] == 1


def test_grow_only_policy(hc):
    assert one(hc, GROW, 100)[:3] == (0, 100, LIVE)
    for n in (100, 7):                                       # equal, smaller: no call, the capacity stays
        e, count, state, s = one(hc, GROW, n)
        assert (e, count, state) == (0, 100, LIVE) and (s["allocs"], s["frees"]) == (0, 0)
    e, count, state, s = one(hc, GROW, 250)                  # larger: a free, then an allocation
    assert (e, count, state) == (0, 250, LIVE) and (s["allocs"], s["frees"], s["bad"], s["peak"]) == (1, 1, 0, 1)
    assert one(hc, GROW, 100)[1] == 250                      # the capacity held is the largest asked for
    assert destroyed_clean(hc)["frees"] == 1


def test_zero_elements_hold_nothing(hc):
    e, count, state, s = one(hc, EXACT, 0)                   # nothing held, nothing wanted: no call
    assert (e, count, state) == (0, 0, NULL) and (s["allocs"], s["frees"]) == (0, 0)
    one(hc, EXACT, 9)
    e, count, state, s = one(hc, EXACT, 0)                   # the buffer is released; the allocator is not asked for 0 bytes
    assert (e, count, state) == (0, 0, NULL) and (s["allocs"], s["frees"], s["bad"]) == (0, 1, 0)
    e, count, state, s = one(hc, GROW, 0)
    assert (e, count, state) == (0, 0, NULL) and (s["allocs"], s["frees"]) == (0, 0)
    e, size, states, s = group(hc, REALLOC, 6, [3, 0, 2, 0, 1])   # a group's member of 0 elements stays null
    assert (e, size, states) == (0, 6, [LIVE, NULL, LIVE, NULL, LIVE]) and s["allocs"] == 3
    assert destroyed_clean(hc)["frees"] == 3


def test_group_policies_free_before_they_allocate(hc):
    counts = [10, 13, 10, 64, 2]
    e, size, states, s = group(hc, EXACT, 10, counts)
    assert (e, size, states) == (0, 10, [LIVE] * MEMBERS) and (s["allocs"], s["frees"]) == (MEMBERS, 0)
    e, size, states, s = group(hc, EXACT, 10, counts)        # the same size: no call
    assert (e, size) == (0, 10) and (s["allocs"], s["frees"]) == (0, 0)
    for want in (4, 30):                                     # smaller, larger: every member freed, then every member allocated
        e, size, states, s = group(hc, EXACT, want, [want, want + 3, want, 64, 2])
        assert (e, size, states) == (0, want, [LIVE] * MEMBERS)
        assert (s["allocs"], s["frees"], s["bad"]) == (MEMBERS, MEMBERS, 0) and s["peak"] == MEMBERS
    e, size, states, s = group(hc, GROW, 12, [12] * MEMBERS)  # grow-only: smaller is no call, the size stays
    assert (e, size) == (0, 30) and (s["allocs"], s["frees"]) == (0, 0)
    e, size, states, s = group(hc, GROW, 31, [31] * MEMBERS)
    assert (e, size, states) == (0, 31, [LIVE] * MEMBERS) and (s["allocs"], s["frees"], s["peak"]) == (MEMBERS, MEMBERS, MEMBERS)
    s = destroyed_clean(hc)
    assert s["frees"] == MEMBERS


@pytest.mark.parametrize("k", range(1, MEMBERS + 1))
@pytest.mark.parametrize("what", [EXACT, GROW, REALLOC])
def test_group_whose_kth_allocation_fails(hc, k, what):
    assert group(hc, what, 8, [8] * MEMBERS)[:2] == (0, 8)
    e, size, states, s = group(hc, what, 20, [20] * MEMBERS, fail_at=k)
    assert e != 0 and size == 0
    assert states == [LIVE] * (k - 1) + [NULL] * (MEMBERS - k + 1)   # every member null or live: none dangles
    assert (s["frees"], s["bad"], s["live"]) == (MEMBERS, 0, k - 1)
    # the next reserve, of ANY size (the old one too: the size reads 0), frees each survivor exactly once and starts again
    e, size, states, s = group(hc, what, 8, [8] * MEMBERS)
    assert (e, size, states) == (0, 8, [LIVE] * MEMBERS)
    assert (s["allocs"], s["frees"], s["bad"], s["live"]) == (MEMBERS, k - 1, 0, MEMBERS)
    # ... and a failure left standing is cleaned up by the destructors alone
    assert group(hc, what, 20, [20] * MEMBERS, fail_at=k)[0] != 0
    s = destroyed_clean(hc)
    assert s["frees"] == k - 1


def test_single_buffer_whose_allocation_fails(hc):
    one(hc, EXACT, 5)
    hc.hc_devbuf_arm(1)
    out = np.zeros(2, np.int64)
    assert hc.hc_devbuf_one(EXACT, 6, out.ctypes.data_as(_i64p)) != 0
    assert (int(out[0]), int(out[1])) == (0, NULL)
    s = stats(hc)
    assert (s["frees"], s["bad"], s["live"]) == (1, 0, 0)
    assert one(hc, EXACT, 6)[:3] == (0, 6, LIVE)
    destroyed_clean(hc)


def test_moved_from_owner_frees_nothing(hc):
    one(hc, EXACT, 16)
    e, count, state, s = one(hc, MOVE)                       # the local that took the block freed it, once; the source holds nothing
    assert (count, state) == (0, NULL) and (s["frees"], s["bad"], s["live"]) == (1, 0, 0)
    s = destroyed_clean(hc)
    assert s["frees"] == 0


def test_pinned_words_are_zeroed(hc):
    hc.hc_devbuf_arm(0)
    assert hc.hc_devbuf_pinned_zeroed(17) == 1
    s = stats(hc)
    assert (s["allocs"], s["frees"], s["bad"], s["live"]) == (1, 1, 0, 0)
