// What the post-processing kernels (pointcloud / cloud_eval / cloud_align / metrics / sample_prep .hip) share: fixed-order sums, ballot ranks,
// the one-block exclusive scan, two host helpers.  Stateless.  NOT in prims.h or common.h: those are built into every eval kernel, and an edit
// there voids the recorded counter traffic of all of them (mvsformer_amd/_sources.py).  The order of the sums is part of the results' bits:
// a wavefront adds by the __shfl_down tree 32, 16, ... 1, a 256-lane block its four wavefronts as (w0 + w1) + (w2 + w3).
#pragma once
#include "common.h"

namespace blk {
// sum over the wavefront, valid in lane 0: double, long long, uint32_t, unsigned long long, float
template <typename T>
__device__ __forceinline__ T wave_sum(T s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    return s;
}
// the four wavefront values of a 256-lane block, combined in the fixed order
template <typename T>
__device__ __forceinline__ T sum4(const T (&w)[4]) { return (w[0] + w[1]) + (w[2] + w[3]); }
// sum over a 256-lane block through the caller's LDS array, valid in every lane; block_sum_put + sum4 are its halves around ONE barrier
template <typename T>
__device__ __forceinline__ void block_sum_put(T v, T (&w)[4]) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
}
template <typename T>
__device__ __forceinline__ T block_sum(T v, T (&w)[4]) {
    block_sum_put(v, w);
    __syncthreads();
    return sum4(w);
}
__device__ __forceinline__ uint32_t ballot_count(bool pred) { return (uint32_t)__popcll(__ballot(pred)); }      // set lanes of the wavefront
// the lane's rank among the set lanes of its wavefront (set lanes below it); wave_count = the wavefront's set lanes
__device__ __forceinline__ uint32_t ballot_rank(bool pred, uint32_t& wave_count) {
    const unsigned long long b = __ballot(pred);
    wave_count = (uint32_t)__popcll(b);
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
}
// block form: the four wavefront counts in LDS (written before a barrier) -> the offset of my wavefront; total = the block's count
__device__ __forceinline__ uint32_t block_rank_offset(const uint32_t (&wcnt)[4], uint32_t& total) {
    const int wave = threadIdx.x >> 6;
    uint32_t woff = 0;
    total = 0;
    for (int w = 0; w < 4; ++w) {
        const uint32_t q = wcnt[w];
        woff += (w < wave) ? q : 0u;
        total += q;
    }
    return woff;
}
// ------------------------------------------------------------------------------------------------------ exclusive scan
constexpr int kScanThreads = 1024, kScanItems = 8;
// ONE block: exclusive 64-bit scan of n uint32 counts in tiles of 1024 * kItems with a running carry; offsets[n] = *total = the sum.
// (templates, the launcher too: only a file that calls it gets the kernel)
template <int kItems>
__global__ __launch_bounds__(kScanThreads) void exclusive_scan_u32_kernel(const uint32_t* __restrict__ counts, long long n,
                                                                                 long long* __restrict__ offsets, long long* __restrict__ total) {
    __shared__ uint32_t wsum[kScanThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    long long carry = 0;
    for (long long base = 0; base < n; base += (long long)kScanThreads * kItems) {
        const long long i0 = base + (long long)t * kItems;
        uint32_t v[kItems], s = 0;
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            v[j] = (i0 + j < n) ? counts[i0 + j] : 0u;
            s += v[j];
        }
        uint32_t inc = s;                                     // inclusive scan over the wavefront; a tile sums to <= 8192 * 256
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint32_t wbase = 0, tile = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) {
            const uint32_t q = wsum[w];
            wbase += (w < wave) ? q : 0u;
            tile += q;
        }
        long long run = carry + (long long)wbase + (long long)(inc - s);
#pragma unroll
        for (int j = 0; j < kItems; ++j)
            if (i0 + j < n) { offsets[i0 + j] = run; run += v[j]; }
        carry += tile;
        __syncthreads();                                      // wsum is rewritten by the next tile
    }
    if (t == 0) {
        offsets[n] = carry;
        if (total) *total = carry;
    }
}
// offsets holds n + 1 entries; total may be null
template <int kItems = kScanItems>
inline void launch_exclusive_scan_u32(const uint32_t* counts, long long n, long long* offsets, long long* total, hipStream_t stream) {
    hipLaunchKernelGGL(exclusive_scan_u32_kernel<kItems>, dim3(1), dim3(kScanThreads), 0, stream, counts, n, offsets, total);
}

inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline unsigned blocks_for(long long n, int per) { return (unsigned)mvs::ceil_div(n, (long long)per); }
}  // namespace blk
