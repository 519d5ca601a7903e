// map_window.h -- the geometry of a map window (graal_map_windows, map_windows.h): the ranks a pixel of a window covers, clipped to the
// genome, the overlap of a pixel's row and column ranks, and the pixel of a rank.  No HIP calls: shared with host_check.cpp, so that the
// CPU tests can hold the clipping and overlap rules to numpy without a device (tests/test_map_windows_cpu.py).
//
// A window is an origin (u0, v0) and a shared (px_rows, px_cols, bin).  Pixel (p, q) covers the row ranks [u0 + p bin, u0 + (p + 1) bin)
// and the column ranks [v0 + q bin, v0 + (q + 1) bin), both cut to [0, S).  Origins may be negative or lie beyond S, and origin + p bin
// may leave int32: the sums are taken in int64.
#pragma once

#if defined(__HIPCC__)
#define MW_HD __host__ __device__ __forceinline__
#else
#define MW_HD inline
#endif

struct MwRange { int lo, hi; };   // the ranks lo .. hi - 1; lo == hi: none

MW_HD int mw_clip(long long r, int S) { return r < 0 ? 0 : r > (long long)S ? S : (int)r; }

// the ranks of pixel p of a side that starts at `origin`
MW_HD MwRange mw_pixel_ranks(int origin, int p, int bin, int S)
{
    const long long lo = (long long)origin + (long long)p * (long long)bin;
    MwRange r;
    r.lo = mw_clip(lo, S);
    r.hi = mw_clip(lo + (long long)bin, S);
    return r;
}

// the ranks of px consecutive pixels from pixel p on (a run of pixels, or with p = 0 a whole side)
MW_HD MwRange mw_span_ranks(int origin, int p, int px, int bin, int S)
{
    const long long lo = (long long)origin + (long long)p * (long long)bin;
    MwRange r;
    r.lo = mw_clip(lo, S);
    r.hi = mw_clip(lo + (long long)px * (long long)bin, S);
    return r;
}

// the ranks two ranges share (empty: lo == hi)
MW_HD MwRange mw_overlap(MwRange a, MwRange b)
{
    MwRange r;
    r.lo = a.lo > b.lo ? a.lo : b.lo;
    r.hi = a.hi < b.hi ? a.hi : b.hi;
    if (r.hi < r.lo) r.hi = r.lo;
    return r;
}

// the pixel of `rank` (in [0, S)) on a side of px pixels that starts at `origin`; -1: outside
MW_HD int mw_pixel_of(int rank, int origin, int px, int bin)
{
    const long long d = (long long)rank - (long long)origin;
    if (d < 0) return -1;
    const long long p = d / (long long)bin;
    return p < (long long)px ? (int)p : -1;
}
