// Cloud alignment for the Tanks-and-Temples protocol (mvsformer_amd/cloud_eval.py: transform, crop_polygon, icp): what a scaled
// point-to-point ICP needs around the nearest-neighbour query of cloud_eval.hip.
//
//   1. mvs_align_transform:     out = round_fp32((r0 x + r1 y) + r2 z + t) per row, in fp64 in exactly this order (no contraction: the build
//                               sets -ffp-contract=off).  ICP transforms the ORIGINAL source by the accumulated fp64 matrix every iteration,
//                               so each coordinate carries one fp32 rounding however many iterations ran.
//   2. mvs_align_crop_polygon:  a slab on one axis and the even-odd crossing rule on the other two, in fp64 from the fp32 coordinates.
//   3. mvs_align_pair_sums:     the sums of one ICP iteration over the pairs (src[i], dst[idx[i]]) with idx >= 0, about an origin, in fp64:
//                               per-lane grid-stride accumulation, a fixed wavefront tree, one row per block; a second single-block launch
//                               folds the rows in index order (eight contiguous chunks, then the chunks in order) and writes ONE record.
// No float atomics, no block waits on another block: two runs over the same input give the same bits.
#include "block_ops.h"

#include <math.h>

#include <algorithm>

namespace {

constexpr int CA_THREADS = 256;
constexpr long long CA_MAX_POINTS = 1LL << 36;
constexpr int CA_MAXK = MVS_ALIGN_CROP_MAX_K;
constexpr int CA_SUMS = 18;                         // sum p (3), sum q (3), sum q p^T (9), sum |p|^2, sum |q|^2, sum dist^2
constexpr int CA_ROW = CA_SUMS + 2;                 // and two counts, carried as bit patterns in the same rows
constexpr int CA_MAX_ROWS = MVS_ALIGN_PAIR_MAX_ROWS;
constexpr int CA_CHUNKS = 8;                        // of the fold: 8 groups of 32 lanes
static_assert(CA_MAX_ROWS % CA_CHUNKS == 0 && CA_ROW <= 32 && CA_THREADS == CA_CHUNKS * 32, "fold layout");

// the device record of the pair sums: MVS_ALIGN_PAIR_RECORD_BYTES = 24 x 8 bytes
struct PairRecord {
    long long n;                                    // pairs: idx in [0, N)
    long long n_finite;                             // rows of src with three finite coordinates
    double s[CA_SUMS];
    long long reserved[4];
};
static_assert(sizeof(PairRecord) == MVS_ALIGN_PAIR_RECORD_BYTES, "PairRecord layout");

struct Affine { double r[3][3]; double t[3]; };
struct Polygon { double u[CA_MAXK]; double v[CA_MAXK]; };
struct Origin { double o[3]; };

using blk::aligned8;
using blk::blocks_for;

// ------------------------------------------------------------------------------------------------------- transform
__global__ __launch_bounds__(CA_THREADS) void align_transform_kernel(const float* __restrict__ pts, long long N, Affine a, float* __restrict__ out) {
    const long long i = (long long)blockIdx.x * CA_THREADS + threadIdx.x;
    if (i >= N) return;
    const double x = (double)pts[3 * i], y = (double)pts[3 * i + 1], z = (double)pts[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[3 * i + r] = (float)((((a.r[r][0] * x) + (a.r[r][1] * y)) + (a.r[r][2] * z)) + a.t[r]);
}

// ------------------------------------------------------------------------------------------------------------ crop
// the polygon sits in the kernel arguments: every lane reads the same vertex, so the loop runs on scalar loads
__global__ __launch_bounds__(CA_THREADS) void align_crop_kernel(const float* __restrict__ pts, long long N, int axis, int ua, int va, double axis_min,
                                                                double axis_max, Polygon poly, int K, uint8_t* __restrict__ mask) {
    const long long i = (long long)blockIdx.x * CA_THREADS + threadIdx.x;
    if (i >= N) return;
    const float fx = pts[3 * i], fy = pts[3 * i + 1], fz = pts[3 * i + 2];
    const double c[3] = {(double)fx, (double)fy, (double)fz};
    const double w = axis == 0 ? c[0] : (axis == 1 ? c[1] : c[2]);
    const double u = ua == 0 ? c[0] : (ua == 1 ? c[1] : c[2]);
    const double v = va == 0 ? c[0] : (va == 1 ? c[1] : c[2]);
    bool inside = false;
    double au = poly.u[K - 1], av = poly.v[K - 1];                          // the closing edge first: (last, first), then (0, 1), ...
    for (int k = 0; k < K; ++k) {
        const double bu = poly.u[k], bv = poly.v[k];
        if ((av > v) != (bv > v)) {                                         // bv != av here: the division is defined
            const double cross = (((bu - au) * (v - av)) / (bv - av)) + au;
            if (u < cross) inside = !inside;
        }
        au = bu;
        av = bv;
    }
    const bool finite = isfinite(fx) && isfinite(fy) && isfinite(fz);
    mask[i] = (finite && axis_min <= w && w <= axis_max && inside) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------- pair sums
__global__ __launch_bounds__(CA_THREADS) void align_pair_sums_kernel(const float* __restrict__ src, long long M, const float* __restrict__ dst,
                                                                     long long N, const long long* __restrict__ idx, const float* __restrict__ dist,
                                                                     Origin og, double* __restrict__ rows) {
    __shared__ double sred[CA_THREADS / 64][CA_ROW];
    double s[CA_SUMS];
#pragma unroll
    for (int k = 0; k < CA_SUMS; ++k) s[k] = 0.0;
    long long n = 0, n_finite = 0;
    for (long long i = (long long)blockIdx.x * CA_THREADS + threadIdx.x; i < M; i += (long long)gridDim.x * CA_THREADS) {
        const float sx = src[3 * i], sy = src[3 * i + 1], sz = src[3 * i + 2];
        n_finite += (isfinite(sx) && isfinite(sy) && isfinite(sz)) ? 1 : 0;
        const long long j = idx[i];
        if (j < 0 || j >= N) continue;                                      // no pair; an index past the target is never dereferenced
        const double d = (double)dist[i];
        const double p[3] = {(double)sx - og.o[0], (double)sy - og.o[1], (double)sz - og.o[2]};
        const double q[3] = {(double)dst[3 * j] - og.o[0], (double)dst[3 * j + 1] - og.o[1], (double)dst[3 * j + 2] - og.o[2]};
        ++n;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s[a] += p[a];
            s[3 + a] += q[a];
#pragma unroll
            for (int b = 0; b < 3; ++b) s[6 + 3 * a + b] += q[a] * p[b];
        }
        s[15] += ((p[0] * p[0]) + (p[1] * p[1])) + (p[2] * p[2]);
        s[16] += ((q[0] * q[0]) + (q[1] * q[1])) + (q[2] * q[2]);
        s[17] += d * d;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < CA_SUMS; ++k) {
        const double w = blk::wave_sum(s[k]);
        if (lane == 0) sred[wave][k] = w;
    }
    n = blk::wave_sum(n);
    n_finite = blk::wave_sum(n_finite);
    if (lane == 0) {
        sred[wave][CA_SUMS] = __longlong_as_double(n);
        sred[wave][CA_SUMS + 1] = __longlong_as_double(n_finite);
    }
    __syncthreads();
    if (threadIdx.x < CA_SUMS) {
        const int k = threadIdx.x;
        rows[(long long)blockIdx.x * CA_ROW + k] = (sred[0][k] + sred[1][k]) + (sred[2][k] + sred[3][k]);
    } else if (threadIdx.x < CA_ROW) {
        const int k = threadIdx.x;
        const long long c = (__double_as_longlong(sred[0][k]) + __double_as_longlong(sred[1][k])) +
                            (__double_as_longlong(sred[2][k]) + __double_as_longlong(sred[3][k]));
        rows[(long long)blockIdx.x * CA_ROW + k] = __longlong_as_double(c);
    }
}

// one block, after the launch above: group g of 32 lanes folds rows [g * chunk, (g + 1) * chunk) in index order, lane k < 20 its column;
// then the eight chunk sums in index order.  chunk depends on the number of rows only.
__global__ __launch_bounds__(CA_THREADS) void align_pair_fold_kernel(const double* __restrict__ rows, int nrows, PairRecord* __restrict__ rec) {
    __shared__ double sred[CA_CHUNKS][CA_ROW];
    const int g = threadIdx.x >> 5, k = threadIdx.x & 31;
    const int chunk = (nrows + CA_CHUNKS - 1) / CA_CHUNKS;
    const int r0 = min(nrows, g * chunk), r1 = min(nrows, r0 + chunk);
    if (k < CA_SUMS) {
        double s = 0.0;
        for (int r = r0; r < r1; ++r) s += rows[(long long)r * CA_ROW + k];
        sred[g][k] = s;
    } else if (k < CA_ROW) {
        long long c = 0;
        for (int r = r0; r < r1; ++r) c += __double_as_longlong(rows[(long long)r * CA_ROW + k]);
        sred[g][k] = __longlong_as_double(c);
    }
    __syncthreads();
    if (threadIdx.x < CA_SUMS) {
        double s = 0.0;
        for (int c = 0; c < CA_CHUNKS; ++c) s += sred[c][threadIdx.x];
        rec->s[threadIdx.x] = s;
    } else if (threadIdx.x < CA_ROW) {
        long long c = 0;
        for (int j = 0; j < CA_CHUNKS; ++j) c += __double_as_longlong(sred[j][threadIdx.x]);
        if (threadIdx.x == CA_SUMS) rec->n = c; else rec->n_finite = c;
    } else if (threadIdx.x < CA_ROW + 4) {
        rec->reserved[threadIdx.x - CA_ROW] = 0;
    }
}

long long pair_rows(long long M) { return std::max<long long>(1, std::min<long long>(CA_MAX_ROWS, mvs::ceil_div(M, (long long)CA_THREADS))); }

}  // namespace

extern "C" int mvs_align_transform(const float* pts, int64_t N, const double* srt_host, float* out, mvs_stream_t stream) {
    MVS_REQUIRE(srt_host && (N == 0 || (pts && out)), "mvs_align_transform: null pointer");
    MVS_REQUIRE(N >= 0 && N <= CA_MAX_POINTS, "mvs_align_transform: N=%lld points", (long long)N);
    if (N == 0) return 0;
    Affine a;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a.r[r][c] = srt_host[3 * r + c];
        a.t[r] = srt_host[9 + r];
    }
    hipLaunchKernelGGL(align_transform_kernel, dim3(blocks_for(N, CA_THREADS)), dim3(CA_THREADS), 0, MVS_STREAM(stream), pts, (long long)N, a, out);
    return mvs::finish_launch("mvs_align_transform");
}

extern "C" int mvs_align_crop_polygon(const float* pts, int64_t N, int axis, double axis_min, double axis_max, const double* polygon_host, int K,
                                      uint8_t* mask, mvs_stream_t stream) {
    MVS_REQUIRE(polygon_host && (N == 0 || (pts && mask)), "mvs_align_crop_polygon: null pointer");
    MVS_REQUIRE(N >= 0 && N <= CA_MAX_POINTS, "mvs_align_crop_polygon: N=%lld points", (long long)N);
    MVS_REQUIRE(axis >= 0 && axis <= 2, "mvs_align_crop_polygon: axis=%d, 0 (X), 1 (Y) or 2 (Z)", axis);
    MVS_REQUIRE(K >= 3 && K <= CA_MAXK, "mvs_align_crop_polygon: K=%d polygon vertices, 3..%d are built", K, CA_MAXK);
    MVS_REQUIRE(!isnan(axis_min) && !isnan(axis_max), "mvs_align_crop_polygon: axis_min / axis_max is NaN");
    Polygon poly;
    for (int k = 0; k < CA_MAXK; ++k) poly.u[k] = poly.v[k] = 0.0;
    for (int k = 0; k < K; ++k) {
        MVS_REQUIRE(isfinite(polygon_host[2 * k]) && isfinite(polygon_host[2 * k + 1]), "mvs_align_crop_polygon: vertex %d is not finite", k);
        poly.u[k] = polygon_host[2 * k];
        poly.v[k] = polygon_host[2 * k + 1];
    }
    if (N == 0) return 0;
    const int ua = axis == 0 ? 1 : 0, va = axis == 2 ? 1 : 2;               // X: (Y, Z)   Y: (X, Z)   Z: (X, Y)
    hipLaunchKernelGGL(align_crop_kernel, dim3(blocks_for(N, CA_THREADS)), dim3(CA_THREADS), 0, MVS_STREAM(stream), pts, (long long)N, axis, ua, va, axis_min,
                       axis_max, poly, K, mask);
    return mvs::finish_launch("mvs_align_crop_polygon");
}

extern "C" int64_t mvs_align_pair_sums_workspace_bytes(int64_t M) {
    if (M < 0 || M > CA_MAX_POINTS) return -1;
    return (int64_t)(8 * CA_ROW * pair_rows((long long)M));
}

extern "C" int mvs_align_pair_sums(const float* src, int64_t M, const float* dst, int64_t N, const int64_t* idx, const float* dist,
                                   const double* origin_host, void* workspace, void* record, mvs_stream_t stream) {
    MVS_REQUIRE(record && workspace && origin_host && (M == 0 || (src && idx && dist)) && (N == 0 || dst), "mvs_align_pair_sums: null pointer");
    MVS_REQUIRE(M >= 0 && M <= CA_MAX_POINTS && N >= 0 && N <= CA_MAX_POINTS, "mvs_align_pair_sums: M=%lld, N=%lld points", (long long)M, (long long)N);
    MVS_REQUIRE(aligned8(record) && aligned8(workspace), "mvs_align_pair_sums: the record and the workspace must be 8-byte aligned");
    Origin og;
    for (int a = 0; a < 3; ++a) {
        MVS_REQUIRE(isfinite(origin_host[a]), "mvs_align_pair_sums: origin[%d] is not finite", a);
        og.o[a] = origin_host[a];
    }
    hipStream_t s = MVS_STREAM(stream);
    double* rows = reinterpret_cast<double*>(workspace);
    const long long nrows = M > 0 ? pair_rows((long long)M) : 0;
    if (nrows > 0)
        hipLaunchKernelGGL(align_pair_sums_kernel, dim3((unsigned)nrows), dim3(CA_THREADS), 0, s, src, (long long)M, dst, (long long)N,
                           reinterpret_cast<const long long*>(idx), dist, og, rows);
    hipLaunchKernelGGL(align_pair_fold_kernel, dim3(1), dim3(CA_THREADS), 0, s, rows, (int)nrows, reinterpret_cast<PairRecord*>(record));
    return mvs::finish_launch("mvs_align_pair_sums");
}
