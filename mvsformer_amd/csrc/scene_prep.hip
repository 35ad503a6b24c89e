// Scene preparation: view selection and depth ranges from a sparse reconstruction (what MVSNet's colmap2mvsnet.py does on the host in a
// double loop over view pairs).  The rule is RESTATED in include/mvs_scene_prep.h (parity with the original script is unverified); this file is
// that text.
//
// Everything hangs on a view-major visibility bitset, bits [V][Wd]: "points seen by i and by j" is a word-wise AND, a row of 10^6 points
// is 125 KB and stays in L2 while the blocks of one i walk their j.  The pair sums use no atomics: one wavefront per pair, one fixed order
// of additions, so S is the same bits on every run.  (The per-point enumeration with fp64 atomics into S is the obvious alternative and
// was not built: its bits move from run to run.)  Integer atomics (the OR that builds the bitset, the two counters of `info`, the LDS
// histograms of the selection) are order-independent.
//
// Bounds: an observation is checked against N and V before its word is addressed; the readers of a bitset mask the last word's bits at
// or above N, so a foreign bitset cannot make them read past xyz; the depth kernel writes a view's segment only after it has checked that
// the segment ends inside `capacity` and that the row holds exactly count[v] bits.
#include "block_ops.h"
#include "../../include/mvs_scene_prep.h"

namespace {

constexpr int SP_THREADS = 256;                    // blk::block_sum / block_rank_offset: four wavefronts
constexpr unsigned SP_MAX_BLOCKS = 1u << 16;       // grid-stride kernels
using u64 = unsigned long long;

__device__ __forceinline__ bool finite3(const float* __restrict__ p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }
// word k of a row without the bits at or above N
__device__ __forceinline__ u64 row_word(const u64* __restrict__ row, long long k, long long N) {
    const u64 w = row[k];
    const long long left = N - k * 64;
    return left >= 64 ? w : (w & ((1ull << left) - 1ull));          // 1 <= left <= 63 in the last word
}

// ---------------------------------------------------------------------------------------------------------------- visibility
__global__ __launch_bounds__(SP_THREADS) void scene_nonfinite_kernel(const float* __restrict__ xyz, long long N, u64* __restrict__ info) {
    __shared__ u64 w[4];
    u64 bad = 0;
    for (long long p = (long long)blockIdx.x * SP_THREADS + threadIdx.x; p < N; p += (long long)gridDim.x * SP_THREADS)
        bad += finite3(xyz + 3 * p) ? 0u : 1u;
    bad = blk::block_sum(bad, w);
    if (threadIdx.x == 0 && bad) atomicAdd(&info[1], bad);
}

__global__ __launch_bounds__(SP_THREADS) void scene_visibility_kernel(const long long* __restrict__ obs_point, const int32_t* __restrict__ obs_view,
                                                                      long long M, const float* __restrict__ xyz, long long N, int V, long long Wd,
                                                                      u64* __restrict__ bits, u64* __restrict__ info) {
    __shared__ u64 w[4];
    u64 bad = 0;
    for (long long m = (long long)blockIdx.x * SP_THREADS + threadIdx.x; m < M; m += (long long)gridDim.x * SP_THREADS) {
        const long long p = obs_point[m];
        const int v = obs_view[m];
        if (p < 0 || p >= N || v < 0 || v >= V) { ++bad; continue; }
        if (finite3(xyz + 3 * p)) atomicOr(&bits[(size_t)v * Wd + (p >> 6)], 1ull << (p & 63));
    }
    bad = blk::block_sum(bad, w);
    if (threadIdx.x == 0 && bad) atomicAdd(&info[0], bad);
}

// one block per view
__global__ __launch_bounds__(SP_THREADS) void scene_row_count_kernel(const u64* __restrict__ bits, long long N, long long Wd, uint32_t* __restrict__ count) {
    __shared__ uint32_t w[4];
    const u64* row = bits + (size_t)blockIdx.x * Wd;
    uint32_t c = 0;
    for (long long k = threadIdx.x; k < Wd; k += SP_THREADS) c += (uint32_t)__popcll(row_word(row, k, N));
    c = blk::block_sum(c, w);
    if (threadIdx.x == 0) count[blockIdx.x] = c;
}

// ---------------------------------------------------------------------------------------------------------------- pair scores
__global__ void scene_centers_kernel(const float* __restrict__ R, const float* __restrict__ t, int V, double* __restrict__ C) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float* r = R + (size_t)v * 9;
    const double t0 = t[3 * v], t1 = t[3 * v + 1], t2 = t[3 * v + 2];
#pragma unroll
    for (int k = 0; k < 3; ++k) C[3 * v + k] = -(((double)r[k] * t0 + (double)r[3 + k] * t1) + (double)r[6 + k] * t2);
}

struct ScoreParams {
    double theta0, sigma1, sigma2;
};

// blockIdx.y = i, one wavefront per j = i + 1 + 4 * blockIdx.x + wave: the four pairs of a block share row i
__global__ __launch_bounds__(SP_THREADS) void scene_pair_scores_kernel(const u64* __restrict__ bits, const float* __restrict__ xyz, long long N, long long Wd,
                                                                       const double* __restrict__ C, int V, ScoreParams q, double* __restrict__ S) {
    const int i = blockIdx.y, lane = threadIdx.x & 63;
    const int j = i + 1 + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (j >= V) return;                                              // the whole wavefront; the kernel has no barrier
    const u64* ri = bits + (size_t)i * Wd;
    const u64* rj = bits + (size_t)j * Wd;
    const double ci0 = C[3 * i], ci1 = C[3 * i + 1], ci2 = C[3 * i + 2];
    const double cj0 = C[3 * j], cj1 = C[3 * j + 1], cj2 = C[3 * j + 2];
    const double deg = 180.0 / 3.141592653589793238462643383279502884;
    double sum = 0.0;
    for (long long k = lane; k < Wd; k += 64) {
        u64 w = row_word(ri, k, N) & rj[k];
        while (w) {
            const int b = __ffsll(w) - 1;
            w &= w - 1ull;
            const float* p = xyz + 3 * (k * 64 + b);
            const double px = p[0], py = p[1], pz = p[2];
            const double a0 = ci0 - px, a1 = ci1 - py, a2 = ci2 - pz;
            const double b0 = cj0 - px, b1 = cj1 - py, b2 = cj2 - pz;
            const double c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
            const double theta = atan2(sqrt((c0 * c0 + c1 * c1) + c2 * c2), (a0 * b0 + a1 * b1) + a2 * b2) * deg;
            const double d = theta - q.theta0, s = theta <= q.theta0 ? q.sigma1 : q.sigma2;
            sum += exp(-(d * d) / (2.0 * s * s));
        }
    }
    sum = blk::wave_sum(sum);
    if (lane == 0) {
        S[(size_t)i * V + j] = sum;
        S[(size_t)j * V + i] = sum;
    }
}

// ---------------------------------------------------------------------------------------------------------------- ranking
// one block per view, its row of S in LDS (V doubles)
__global__ __launch_bounds__(SP_THREADS) void scene_rank_kernel(const double* __restrict__ S, int V, int k, int32_t* __restrict__ src,
                                                                double* __restrict__ score) {
    extern __shared__ double row[];
    const int i = blockIdx.x;
    for (int m = threadIdx.x; m < V; m += SP_THREADS) row[m] = S[(size_t)i * V + m];
    for (int r = threadIdx.x; r < k; r += SP_THREADS) {
        src[(size_t)i * k + r] = -1;
        score[(size_t)i * k + r] = 0.0;
    }
    __syncthreads();                                                 // the row is complete; the fill is behind every lane's later store
    for (int j = threadIdx.x; j < V; j += SP_THREADS) {
        if (j == i) continue;
        const double sj = row[j];
        int rank = 0;
        for (int m = 0; m < V; ++m) {
            const double sm = row[m];
            rank += (m != i && (sm > sj || (sm == sj && m < j))) ? 1 : 0;
        }
        if (rank < k) {
            src[(size_t)i * k + rank] = j;
            score[(size_t)i * k + rank] = sj;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- depth ranges
// order-preserving key of a float: ascending keys = ascending floats, negative ones first
__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t key) { return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key); }

// one block per view: compaction of its depths in ascending point order, then the exact selection of two order statistics
__global__ __launch_bounds__(SP_THREADS) void scene_depth_ranges_kernel(const u64* __restrict__ bits, const uint32_t* __restrict__ count,
                                                                        const float* __restrict__ xyz, long long N, long long Wd,
                                                                        const float* __restrict__ R, const float* __restrict__ t, double lo, double hi,
                                                                        const long long* __restrict__ offsets, float* depths, long long capacity,
                                                                        float* __restrict__ range, int32_t* __restrict__ nout) {
    __shared__ uint32_t wcnt[4];
    __shared__ uint32_t hist[2][256];
    __shared__ uint32_t sel[2][2];                                   // per order statistic: the key's digits found so far, the rank left inside them
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64* row = bits + (size_t)v * Wd;
    const long long off = offsets[v];
    const uint32_t n = count[v];
    // a wavefront owns a contiguous quarter of the row: its offset inside the segment is the popcount of the quarters before it
    const long long per = (Wd + 3) / 4, k0 = wave * per, k1 = min(Wd, k0 + per);
    uint32_t c = 0;
    for (long long k = k0 + lane; k < k1; k += 64) c += (uint32_t)__popcll(row_word(row, k, N));
    blk::block_sum_put(c, wcnt);
    __syncthreads();
    uint32_t total;
    uint32_t base = blk::block_rank_offset(wcnt, total);
    const bool fits = off >= 0 && off + (long long)n <= capacity && total == n;
    if (n == 0 || !fits) {                                           // the whole block
        if (tid == 0) {
            range[2 * v] = 0.0f;
            range[2 * v + 1] = 0.0f;
            nout[v] = fits ? 0 : -1;
        }
        return;
    }
    const float r20 = R[(size_t)v * 9 + 6], r21 = R[(size_t)v * 9 + 7], r22 = R[(size_t)v * 9 + 8], t2 = t[3 * v + 2];
    float* seg = depths + off;
    for (long long k = k0; k < k1; ++k) {                            // wave-uniform: the lanes are the 64 points of word k
        const u64 w = row_word(row, k, N);
        if (w == 0) continue;
        const bool set = (w >> lane) & 1ull;
        uint32_t wave_count;
        const uint32_t r = blk::ballot_rank(set, wave_count);
        if (set) {
            const float* p = xyz + 3 * (k * 64 + lane);
            seg[base + r] = ((r20 * p[0] + r21 * p[1]) + r22 * p[2]) + t2;      // base + r < total == n
        }
        base += wave_count;
    }
    if (tid < 2) {
        const long long want = (long long)((double)n * (tid ? hi : lo));
        sel[tid][0] = 0;
        sel[tid][1] = (uint32_t)min(max(want, 0ll), (long long)n - 1);
    }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t above = pass ? (0xFFFFFFFFu << (shift + 8)) : 0u;       // the digits already fixed
        hist[0][tid] = 0;
        hist[1][tid] = 0;
        __syncthreads();                                             // the segment (first pass), sel and the cleared bins are visible
        const uint32_t pre0 = sel[0][0], pre1 = sel[1][0];
        for (uint32_t e = tid; e < n; e += SP_THREADS) {
            const uint32_t key = float_key(seg[e]);
            const uint32_t digit = (key >> shift) & 255u;
            if ((key & above) == pre0) atomicAdd(&hist[0][digit], 1u);
            if ((key & above) == pre1) atomicAdd(&hist[1][digit], 1u);
        }
        __syncthreads();
        if (tid < 2) {                                               // the bin that holds rank sel[tid][1]: always found, the bins sum to more than it
            uint32_t left = sel[tid][1], d = 0;
            for (; d < 255u; ++d) {
                const uint32_t h = hist[tid][d];
                if (left < h) break;
                left -= h;
            }
            sel[tid][0] |= d << shift;
            sel[tid][1] = left;
        }
        __syncthreads();                                             // the bins are read before the next pass clears them
    }
    if (tid < 2) range[2 * v + tid] = key_float(sel[tid][0]);
    if (tid == 0) nout[v] = (int32_t)n;
}

bool scene_shape_ok(int64_t N, int V) { return V >= 1 && V <= MVS_SCENE_MAX_VIEWS && N >= 1 && N < (1ll << 31); }

}  // namespace

extern "C" int mvs_scene_visibility(const int64_t* obs_point, const int32_t* obs_view, int64_t M, const float* xyz, int64_t N, int V, uint64_t* bits,
                                   uint32_t* count, int64_t* info, int64_t* info_host, mvs_stream_t stream) {
    MVS_REQUIRE(xyz && bits && count && info && (M == 0 || (obs_point && obs_view)), "mvs_scene_visibility: null pointer");
    MVS_REQUIRE(scene_shape_ok(N, V) && M >= 0 && M < (1ll << 32), "mvs_scene_visibility: bad shape N=%lld M=%lld V=%d (1 <= V <= %d, 1 <= N < 2^31, 0 <= M < 2^32)",
                (long long)N, (long long)M, V, MVS_SCENE_MAX_VIEWS);
    MVS_REQUIRE(blk::aligned8(bits) && blk::aligned8(info), "mvs_scene_visibility: bits and info must be 8-byte aligned");
    hipStream_t s = MVS_STREAM(stream);
    const long long Wd = mvs::ceil_div((long long)N, 64ll);
    u64* b = reinterpret_cast<u64*>(bits);
    u64* inf = reinterpret_cast<u64*>(info);
    if (hipMemsetAsync(bits, 0, sizeof(u64) * (size_t)V * (size_t)Wd, s) != hipSuccess || hipMemsetAsync(info, 0, 2 * sizeof(int64_t), s) != hipSuccess)
        return mvs::finish_launch("mvs_scene_visibility(memset)");
    hipLaunchKernelGGL(scene_nonfinite_kernel, dim3(min(blk::blocks_for(N, SP_THREADS), SP_MAX_BLOCKS)), dim3(SP_THREADS), 0, s, xyz, (long long)N, inf);
    if (M > 0)
        hipLaunchKernelGGL(scene_visibility_kernel, dim3(min(blk::blocks_for(M, SP_THREADS), SP_MAX_BLOCKS)), dim3(SP_THREADS), 0, s,
                           reinterpret_cast<const long long*>(obs_point), obs_view, (long long)M, xyz, (long long)N, V, Wd, b, inf);
    hipLaunchKernelGGL(scene_row_count_kernel, dim3(V), dim3(SP_THREADS), 0, s, b, (long long)N, Wd, count);
    if (int rc = mvs::finish_launch("mvs_scene_visibility")) return rc;
    if (!info_host) return MVS_OK;
    if (hipMemcpyAsync(info_host, info, 2 * sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return mvs::finish_launch("mvs_scene_visibility(copy)");
    MVS_REQUIRE(info_host[0] == 0, "mvs_scene_visibility: %lld observations name a point outside [0, %lld) or a view outside [0, %d)",
                (long long)info_host[0], (long long)N, V);
    return MVS_OK;
}

extern "C" int mvs_scene_pair_scores(const uint64_t* bits, const float* xyz, int64_t N, const float* R, const float* t, int V, double theta0,
                                    double sigma1, double sigma2, double* centers, double* S, mvs_stream_t stream) {
    MVS_REQUIRE(bits && xyz && R && t && centers && S, "mvs_scene_pair_scores: null pointer");
    MVS_REQUIRE(scene_shape_ok(N, V), "mvs_scene_pair_scores: bad shape N=%lld V=%d (1 <= V <= %d, 1 <= N < 2^31)", (long long)N, V, MVS_SCENE_MAX_VIEWS);
    MVS_REQUIRE(theta0 == theta0 && sigma1 > 0.0 && sigma2 > 0.0, "mvs_scene_pair_scores: theta0 is NaN or a sigma is not positive (%g, %g, %g)", theta0,
                sigma1, sigma2);
    MVS_REQUIRE(blk::aligned8(bits) && blk::aligned8(centers) && blk::aligned8(S), "mvs_scene_pair_scores: bits, centers and S must be 8-byte aligned");
    hipStream_t s = MVS_STREAM(stream);
    if (hipMemsetAsync(S, 0, sizeof(double) * (size_t)V * V, s) != hipSuccess) return mvs::finish_launch("mvs_scene_pair_scores(memset)");
    hipLaunchKernelGGL(scene_centers_kernel, dim3(mvs::ceil_div(V, 64)), dim3(64), 0, s, R, t, V, centers);
    if (V > 1)
        hipLaunchKernelGGL(scene_pair_scores_kernel, dim3(mvs::ceil_div(V - 1, 4), V), dim3(SP_THREADS), 0, s, reinterpret_cast<const u64*>(bits), xyz,
                           (long long)N, mvs::ceil_div((long long)N, 64ll), centers, V, ScoreParams{theta0, sigma1, sigma2}, S);
    return mvs::finish_launch("mvs_scene_pair_scores");
}

extern "C" int mvs_scene_rank_sources(const double* S, int V, int k, int32_t* src, double* score, mvs_stream_t stream) {
    MVS_REQUIRE(S && src && score, "mvs_scene_rank_sources: null pointer");
    MVS_REQUIRE(V >= 1 && V <= MVS_SCENE_MAX_VIEWS && k >= 1 && k <= (1 << 20), "mvs_scene_rank_sources: bad shape V=%d k=%d (1 <= V <= %d, k >= 1)", V, k,
                MVS_SCENE_MAX_VIEWS);
    hipLaunchKernelGGL(scene_rank_kernel, dim3(V), dim3(SP_THREADS), sizeof(double) * (size_t)V, MVS_STREAM(stream), S, V, k, src, score);
    return mvs::finish_launch("mvs_scene_rank_sources");
}

extern "C" int mvs_scene_depth_ranges(const uint64_t* bits, const uint32_t* count, const float* xyz, int64_t N, const float* R, const float* t, int V,
                                     double lo, double hi, int64_t* offsets, float* depths, int64_t capacity, float* range, int32_t* n,
                                     mvs_stream_t stream) {
    MVS_REQUIRE(bits && count && xyz && R && t && offsets && range && n && (depths || capacity == 0), "mvs_scene_depth_ranges: null pointer");
    MVS_REQUIRE(scene_shape_ok(N, V) && capacity >= 0, "mvs_scene_depth_ranges: bad shape N=%lld V=%d capacity=%lld (1 <= V <= %d, 1 <= N < 2^31)",
                (long long)N, V, (long long)capacity, MVS_SCENE_MAX_VIEWS);
    MVS_REQUIRE(lo >= 0.0 && lo <= hi && hi <= 1.0, "mvs_scene_depth_ranges: 0 <= lo <= hi <= 1, got lo=%g hi=%g", lo, hi);
    MVS_REQUIRE(blk::aligned8(bits) && blk::aligned8(offsets), "mvs_scene_depth_ranges: bits and offsets must be 8-byte aligned");
    hipStream_t s = MVS_STREAM(stream);
    long long* off = reinterpret_cast<long long*>(offsets);
    blk::launch_exclusive_scan_u32(count, V, off, nullptr, s);
    hipLaunchKernelGGL(scene_depth_ranges_kernel, dim3(V), dim3(SP_THREADS), 0, s, reinterpret_cast<const u64*>(bits), count, xyz, (long long)N,
                       mvs::ceil_div((long long)N, 64ll), R, t, lo, hi, off, depths, (long long)capacity, range, n);
    return mvs::finish_launch("mvs_scene_depth_ranges");
}
