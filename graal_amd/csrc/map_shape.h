// map_shape.h -- the binning of a layout map (graal_layout_maps, maps.h): how many consecutive sub-fragments of the genome order share a
// pixel, how many pixels a side has, and the pixel of a rank.  image.matrix_image's rule, exactly.  No HIP calls: shared with
// host_check.cpp, so that the CPU tests can check it without a device (tests/test_maps_cpu.py).
#pragma once

#if defined(__HIPCC__)
#define MS_HD __host__ __device__ __forceinline__
#else
#define MS_HD inline
#endif

struct MapShape { int bin, m; };

// S ranked sub-fragments on at most max_px pixels a side (S >= 0, max_px >= 1)
MS_HD MapShape map_shape(int S, int max_px)
{
    MapShape r;
    const int per = (S + max_px - 1) / max_px;
    r.bin = per > 1 ? per : 1;
    r.m = (S + r.bin - 1) / r.bin;
    return r;
}

MS_HD int map_pixel(int rank, int bin) { return rank / bin; }
