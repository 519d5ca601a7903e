// wave_runs.h -- segmented sums over a wave's runs of equal keys (a run: consecutive lanes with one key): what the contact streams and
// the tile walks do before their atomics.  Included by graal_hip.hip before score_common.h; it needs nothing but the wave size.  Every
// function is for the WHOLE wave, under wave-uniform control flow, and leaves a run's sum in the run's LAST lane (the tail).
//   head form, for many sums over the same key: run_head / run_tail once, then run_sum(v, head) per value;
//   flag form, for one pass: run_sums(key, tail, v...), any number of values together.
#pragma once

namespace {

// the lane at which the run that holds this lane begins
template <class K>
__device__ __forceinline__ int run_head(K key)
{
    const int lane = threadIdx.x & 63;
    const K kp = __shfl_up(key, 1, 64);
    int h = (lane == 0 || kp != key) ? lane : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int hu = __shfl_up(h, o, 64);
        if (lane >= o) h = max(h, hu);
    }
    return h;
}

// whether this lane is its run's last (by every lane: a shuffle reads nothing from a lane that skips it)
template <class K>
__device__ __forceinline__ bool run_tail(K key)
{
    const K kn = __shfl_down(key, 1, 64);
    return (threadIdx.x & 63) == 63 || kn != key;
}

// segmented inclusive sum, the run's head lane known
__device__ __forceinline__ long long run_sum(long long v, int head)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long vu = __shfl_up(v, o, 64);
        if (lane - o >= head) v += vu;
    }
    return v;
}

// flag form: on return every `v` of a run's last lane (`tail`) holds the run's sum
template <class K, class... V>
__device__ __forceinline__ void run_sums(K key, bool& tail, V&... v)
{
    static_assert((... && std::is_same_v<V, long long>), "run_sums: long long values");
    const int lane = threadIdx.x & 63;
    const K kp = __shfl_up(key, 1, 64), kn = __shfl_down(key, 1, 64);
    int f = (lane == 0 || kp != key) ? 1 : 0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long u[] = { __shfl_up(v, o, 64)... };
        const int fu = __shfl_up(f, o, 64);
        if (lane >= o && !f) { int i = 0; ((v += u[i++]), ...); f |= fu; }
    }
    tail = lane == 63 || kn != key;
}

} // namespace
