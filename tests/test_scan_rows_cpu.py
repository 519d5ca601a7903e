"""CPU: the host side of the contact list's row index (graal_amd/csrc/scan_rows.h, compiled for the host into the test-only
library): the upload's sortedness check and longest row, the row offsets against np.searchsorted, the bound on the rows a step
can affect and the switch between the streaming and the indexed producer."""
import ctypes

import numpy as np

from graal_amd import synth
from tests import util

_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)


def hc():
    L = util.hostcheck()
    L.hc_row_index.restype = None
    L.hc_row_index.argtypes = [_i32p, ctypes.c_int64, ctypes.c_int32, _i64p, _i64p]
    L.hc_scan_rows_bound.restype = ctypes.c_int64
    L.hc_scan_rows_bound.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int]
    L.hc_scan_rows_wins.restype = ctypes.c_int
    L.hc_scan_rows_wins.argtypes = [ctypes.c_int64] * 4
    L.hc_scan_rows_cap.restype = ctypes.c_int
    return L


def row_index(row, S):
    row = np.ascontiguousarray(row, dtype=np.int32)
    out = np.zeros(2, np.int64)
    rowptr = np.full(S + 1, -1, np.int64)
    hc().hc_row_index(row.ctypes.data_as(_i32p), len(row), S, out.ctypes.data_as(_i64p), rowptr.ctypes.data_as(_i64p))
    return bool(out[0]), int(out[1]), rowptr


def test_row_offsets_of_a_sorted_list_equal_searchsorted():
    for n_sub, seed in ((1, 1), (3, 2)):
        P = synth.make_problem(n_bins=300, nnz=20000, n_sub=n_sub, seed=seed, contig_weights=(5, 3, 2), mean_len_bp=1500.0,
                               accu=1 if n_sub == 1 else 9, param=synth.make_param_simu(fact=300.0, v_inter=0.03))
        row, S = P["coo_row"], int(P["init_n_sub_frags"])
        srt, longest, rowptr = row_index(row, S)
        assert srt
        assert longest == np.bincount(row, minlength=S).max()
        assert np.array_equal(rowptr, np.searchsorted(row, np.arange(S + 1), side="left"))
        assert rowptr[0] == 0 and rowptr[S] == len(row)
        assert rowptr[S - 1] == len(row)          # the last id is never a row (row < col): its slice is empty


def test_edges_of_the_row_index():
    srt, longest, rowptr = row_index(np.zeros(0, np.int32), 4)
    assert srt and longest == 0 and np.array_equal(rowptr, np.zeros(5, np.int64))
    srt, longest, rowptr = row_index(np.array([2, 2, 2, 5], np.int32), 7)      # empty rows in front, between and behind
    assert srt and longest == 3 and list(rowptr) == [0, 0, 0, 3, 3, 3, 4, 4]
    srt, longest, rowptr = row_index(np.array([0, 1, 1, 0], np.int32), 3)       # one step down: no index
    assert not srt and np.all(rowptr == -1)
    rng = np.random.RandomState(3)
    row = np.sort(rng.randint(0, 50, size=500)).astype(np.int32)
    assert row_index(row, 50)[0] and not row_index(row[::-1].copy(), 50)[0]


def test_bound_and_switch():
    L = hc()
    cap = L.hc_scan_rows_cap()
    assert cap == 2048
    assert L.hc_scan_rows_bound(5, 12, 1) == 6 * 12 and L.hc_scan_rows_bound(5, 12, 0) == 6 * 12 * 3
    assert L.hc_scan_rows_bound(10, 0, 1) == 11      # (a longest contig of at least one fragment)
    # the benchmark's exploded layout: longest contig 5 -> at most 2 * 5 + 2 between relabels, longest row 557, 20 M contacts
    rows = L.hc_scan_rows_bound(5, 12, 1)
    assert rows * 557 == 40104 and L.hc_scan_rows_wins(rows, 557, 20_000_000, 16) == 1
    # its late stage (contigs of thousands of fragments): more rows than the pass's list holds
    assert L.hc_scan_rows_wins(L.hc_scan_rows_bound(5, 6800, 1), 557, 20_000_000, 16) == 0
    # the switch itself: rows x longest row x R <= nnz
    assert L.hc_scan_rows_wins(100, 100, 160_000, 16) == 1 and L.hc_scan_rows_wins(100, 100, 159_999, 16) == 0
    assert L.hc_scan_rows_wins(cap, 1, 10 ** 9, 16) == 1 and L.hc_scan_rows_wins(cap + 1, 1, 10 ** 9, 16) == 0
    assert L.hc_scan_rows_wins(10, 0, 160, 16) == 1     # (an empty longest row counts as one contact)
