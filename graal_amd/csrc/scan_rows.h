// Host side of the row index of the contact list (k_scan_rows): the sortedness check and the longest row of the upload, the row offsets'
// binary search, the bound on the rows a step can affect and the switch between the two producers.  Shared with host_check.cpp, so that
// the CPU tests can check them without a device (tests/test_scan_rows_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SR_HD __host__ __device__ __forceinline__
#else
#define SR_HD inline
#endif

// over the upload's host loop: is `row` non-decreasing, and how long is its longest run of equal ids (sorted: the longest row)
struct RowRuns {
    bool sorted = true;
    long long run = 0, longest = 0;
    int prev = -1;
    inline void add(int r)
    {
        if (r < prev) sorted = false;
        run = (r == prev) ? run + 1 : 1;
        if (run > longest) longest = run;
        prev = r;
    }
};

// first contact of row >= s (`row` sorted): rowptr[s]
SR_HD long long row_lower_bound(const int* row, long long nnz, int s)
{
    long long lo = 0, hi = nnz;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (row[mid] < s) lo = mid + 1; else hi = mid;
    }
    return lo;
}

constexpr int ROWS_CAP = 2048;   // affected rows a step of the indexed pass may have (k_scan_rows' LDS list)

// bound on the rows a step can affect: K + 1 contigs of at most lc fragments, every sub-fragment of a bin a row of its own
inline long long scan_rows_bound(int K, long long lc, bool single_sub) { return (long long)(K + 1) * (lc < 1 ? 1 : lc) * (single_sub ? 1 : 3); }

// the switch: the rows fit the kernel's list and the contacts the pass can visit at worst, rows x longest row, are at most nnz / R
inline bool scan_rows_wins(long long rows, long long longest_row, long long nnz, long long R)
{
    return rows <= (long long)ROWS_CAP && rows * (longest_row < 1 ? 1 : longest_row) * R <= nnz;
}
