// Point-cloud evaluation: nearest-neighbour distances between two clouds, voxel thinning and the score reduction behind DTU's
// accuracy / completeness and Tanks-and-Temples' precision / recall / F-score (mvsformer_amd/cloud_eval.py).
//
// A uniform grid over the TARGET cloud: the cell of a point is floorf((x - origin) / cell) per axis - these two fp32 operations, in this
// order; origin = the cloud's per-axis minimum (bounds_kernel: integer atomics on order-preserving bit patterns, so min and max are
// exact and order-free).  A cell's key is x | y << 21 | z << 42: x runs fastest, the cells of one x-row are consecutive keys and, after
// the sort, consecutive points - one range lookup serves the whole row of a shell.
//
//   1. mvs_cloud_bounds:      min / max over the finite points, the number of non-finite ones; the caller reads 32 bytes.
//   2. mvs_cloud_grid_keys:   one int64 key per point (non-finite points: the largest key, behind every cell).
//      ... the caller sorts the keys (stable) and keeps the permutation ...
//   3. mvs_cloud_grid_build:  heads of runs of equal keys -> count per 256-point block -> one-block scan (block_ops.h) -> scatter: the table of
//                             occupied cells (key, first point), and the points gathered into cell order.  Stable: the permutation of
//                             a stable sort keeps the original order inside a cell.
//   4. mvs_cloud_nn_query:    one lane per query, queries in cell order (their own sorted keys): Chebyshev shells of cells around the
//                             query's cell until the lower bound of everything not yet visited reaches the best distance or max_dist.
//   5. mvs_cloud_voxel_*:     the same table with cell = voxel: one lane per occupied voxel adds its points in double in original order.
//   6. mvs_cloud_score:       counts below max_dist and below each tau (ballot + popcount, 64-bit integer atomics), the distances below
//                             max_dist added in double per block, the block sums added in a fixed order by a second launch.
//   7. mvs_greedy_thin:       DTU's thinning over the same table with cell >= dist (neighbours lie in the 3 x 3 x 3 cells around a point):
//                             rounds over the points still undecided, one launch each; the host reads a counter per batch of rounds.
// No float atomics, no block waits on another block, every phase is its own launch on one stream.
//
// Exactness of the search.  The cell of a point is computed in fp32, so a cell is not an exact box: with u = fl(fl(x - origin) / cell)
// and u* the real quotient, |u - u*| <= 2^-23 |u*| (two roundings).  Two points whose cells differ by s + 1 or more on an axis are
// therefore farther apart than (s - slack) * cell with slack = 2^-22 * 1.01 * (largest |u| in play).  The walk uses that bound, shrunk by
// another 1e-5 relative to cover the fp32 rounding of the distance itself: it never skips a point the brute-force scan would pick.
#include "block_ops.h"

#include <math.h>
#include <string.h>

#include <algorithm>

namespace {

using blk::aligned8;
using blk::blocks_for;

constexpr int CE_THREADS = 256;
constexpr int CE_AXIS_BITS = 21;
constexpr long long CE_AXIS_CELLS = 1LL << CE_AXIS_BITS;                  // MVS_CLOUD_MAX_AXIS_CELLS
constexpr long long CE_BAD_KEY = 0x7fffffffffffffffLL;                    // non-finite points: behind every cell after the sort
constexpr long long CE_MAX_POINTS = 1LL << 36;
constexpr int CE_MAXK = MVS_CLOUD_SCORE_MAX_K;

// the device record of a grid: MVS_CLOUD_GRID_RECORD_BYTES
struct CloudGrid {
    uint32_t lo_bits[3], hi_bits[3];      // order-preserving patterns of the per-axis min / max over the finite points
    float origin[3];                      // = the minimum (0 for a cloud without a finite point)
    float cell;
    int32_t ncell[3];                     // occupied extent in cells per axis: floorf((max - origin) / cell) + 1
    int32_t reserved;
    long long n_bad;                      // non-finite points
    long long n_valid;                    // points in the index
    long long n_cells;                    // occupied cells
};
static_assert(sizeof(CloudGrid) <= MVS_CLOUD_GRID_RECORD_BYTES, "CloudGrid layout");

// the device record of a score: MVS_CLOUD_SCORE_RECORD_BYTES = 16 x 8 bytes
struct CloudScore {
    long long n;                          // distances given
    long long n_below;                    // distances < max_dist
    long long below_tau[CE_MAXK];         // distances < tau[k]
    double sum;                           // sum of the distances < max_dist
    double mean;                          // sum / n_below (NaN for an empty set)
    long long reserved[4];
};
static_assert(sizeof(CloudScore) == MVS_CLOUD_SCORE_RECORD_BYTES, "CloudScore layout");

struct Taus { float t[CE_MAXK]; };

__device__ __forceinline__ uint32_t order_bits(float f) {                  // a < b  <=>  order_bits(a) < order_bits(b) (finite values)
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float from_order_bits(uint32_t b) {
    const uint32_t u = (b & 0x80000000u) ? (b & 0x7fffffffu) : ~b;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the cell rule: two IEEE fp32 operations and a floor (no contraction: the build sets -ffp-contract=off)
__host__ __device__ inline float cell_coord(float x, float origin, float cell) { return floorf((x - origin) / cell); }

__device__ __forceinline__ long long make_key(int cx, int cy, int cz) {
    return (long long)cx | ((long long)cy << CE_AXIS_BITS) | ((long long)cz << (2 * CE_AXIS_BITS));
}

// the cell of an indexed point.  origin = the minimum, ncell sized from the maximum by the same monotone operations: 0 <= c < ncell <= 2^21;
// the clamp only guards a caller whose bounds do not belong to these points
struct Cell { int x, y, z; };
__device__ __forceinline__ Cell own_cell(float x, float y, float z, const float (&origin)[3], float cell, const int (&ncell)[3]) {
    return Cell{min(max((int)cell_coord(x, origin[0], cell), 0), ncell[0] - 1), min(max((int)cell_coord(y, origin[1], cell), 0), ncell[1] - 1),
                min(max((int)cell_coord(z, origin[2], cell), 0), ncell[2] - 1)};
}

// ---------------------------------------------------------------------------------------------------------- bounds
__global__ __launch_bounds__(CE_THREADS) void cloud_bounds_kernel(const float* __restrict__ pts, long long N, CloudGrid* __restrict__ g) {
    __shared__ uint32_t slo[3][CE_THREADS / 64], shi[3][CE_THREADS / 64], sbad[CE_THREADS / 64];
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    uint32_t bad = 0;
    for (long long i = (long long)blockIdx.x * CE_THREADS + threadIdx.x; i < N; i += (long long)gridDim.x * CE_THREADS) {
        const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        if (finite3(x, y, z)) {
            const uint32_t b[3] = {order_bits(x), order_bits(y), order_bits(z)};
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], b[a]); hi[a] = max(hi[a], b[a]); }
        } else {
            ++bad;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {                                      // the count rides in the min / max tree: its own pass costs registers
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = min(lo[a], (uint32_t)__shfl_down(lo[a], o, 64));
            hi[a] = max(hi[a], (uint32_t)__shfl_down(hi[a], o, 64));
        }
        bad += __shfl_down(bad, o, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { slo[a][wave] = lo[a]; shi[a][wave] = hi[a]; }
        sbad[wave] = bad;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        uint32_t l = slo[a][0], h = shi[a][0];
        for (int w = 1; w < CE_THREADS / 64; ++w) { l = min(l, slo[a][w]); h = max(h, shi[a][w]); }
        atomicMin(&g->lo_bits[a], l);
        atomicMax(&g->hi_bits[a], h);
    } else if (threadIdx.x == 3) {
        const uint32_t b = blk::sum4(sbad);
        if (b) atomicAdd(reinterpret_cast<unsigned long long*>(&g->n_bad), (unsigned long long)b);
    }
}

// ------------------------------------------------------------------------------------------------------------ keys
struct GridSetup { float origin[3]; float cell; int ncell[3]; long long n_valid; };

__global__ __launch_bounds__(CE_THREADS) void cloud_keys_kernel(const float* __restrict__ pts, long long N, GridSetup s, CloudGrid* __restrict__ g,
                                                                long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (i == 0) {                                                           // the record the later launches read
#pragma unroll
        for (int a = 0; a < 3; ++a) { g->origin[a] = s.origin[a]; g->ncell[a] = s.ncell[a]; }
        g->cell = s.cell;
        g->n_valid = s.n_valid;
        g->n_cells = 0;
    }
    if (i >= N) return;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    long long key = CE_BAD_KEY;
    if (finite3(x, y, z)) {
        const Cell c = own_cell(x, y, z, s.origin, s.cell, s.ncell);
        key = make_key(c.x, c.y, c.z);
    }
    keys[i] = key;
}

// a query's cell in the TARGET's grid, clamped to +-2^22 per axis (a query that far out has no target within any allowed max_dist)
__device__ __forceinline__ int query_coord(float x, float origin, float cell) {
    const float u = cell_coord(x, origin, cell);
    return (int)fminf(fmaxf(u, -4194304.0f), 4194304.0f);
}

// queries are only ORDERED by these keys (lanes of a wavefront then walk the same cells): clamped into the grid, non-finite ones last
__global__ __launch_bounds__(CE_THREADS) void cloud_query_keys_kernel(const float* __restrict__ q, long long M, const CloudGrid* __restrict__ g,
                                                                      long long* __restrict__ keys) {
    const long long i = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (i >= M) return;
    const float x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
    long long key = CE_BAD_KEY;
    if (finite3(x, y, z)) {
        const int top = (int)CE_AXIS_CELLS - 1;
        const int cx = min(max(query_coord(x, g->origin[0], g->cell), 0), top);
        const int cy = min(max(query_coord(y, g->origin[1], g->cell), 0), top);
        const int cz = min(max(query_coord(z, g->origin[2], g->cell), 0), top);
        key = make_key(cx, cy, cz);
    }
    keys[i] = key;
}

// ------------------------------------------------------------------------------------------------------------ build
// workspace: offsets int64 [nb + 1], then counts uint32 [nb], nb = ceil(N / 256)
__device__ __forceinline__ bool is_head(const long long* __restrict__ sk, long long i, long long n_valid) {
    return i < n_valid && (i == 0 || sk[i] != sk[i - 1]);
}

__global__ __launch_bounds__(CE_THREADS) void cloud_heads_count_kernel(const long long* __restrict__ sk, long long N, const CloudGrid* __restrict__ g,
                                                                       uint32_t* __restrict__ counts) {
    __shared__ uint32_t part[CE_THREADS / 64];
    const long long i = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    const bool h = i < N && is_head(sk, i, g->n_valid);
    const uint32_t c = blk::ballot_count(h);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = blk::sum4(part);
}

// The scatter.  Lane 0 of block 0 also closes the table: cell_start[n_cells] = n_valid, n_cells = offsets[nb] as the scan left it
// (n_cells <= N: cell_start holds N + 1 entries; no other lane of this launch writes that entry, and the first reader is a later launch).
__global__ __launch_bounds__(CE_THREADS) void cloud_build_kernel(const float* __restrict__ pts, long long N, const long long* __restrict__ sk,
                                                                 const long long* __restrict__ perm, const CloudGrid* __restrict__ g,
                                                                 const long long* __restrict__ offsets, float* __restrict__ sorted_pts,
                                                                 long long* __restrict__ cell_keys, long long* __restrict__ cell_start) {
    __shared__ uint32_t wcnt[CE_THREADS / 64];
    const long long i = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    const long long n_valid = g->n_valid;
    const bool h = i < N && is_head(sk, i, n_valid);
    uint32_t wave_cnt, block_cnt;
    const uint32_t rank = blk::ballot_rank(h, wave_cnt);
    if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = wave_cnt;
    __syncthreads();
    const uint32_t woff = blk::block_rank_offset(wcnt, block_cnt);
    if (h) {
        const long long c = offsets[blockIdx.x] + (long long)(woff + rank);
        if (c >= 0 && c < N) { cell_keys[c] = sk[i]; cell_start[c] = i; }   // never past what the caller allocated
    }
    if (sorted_pts && i < N && i < n_valid) {
        const long long src = perm[i];
        if (src >= 0 && src < N) {
            sorted_pts[3 * i] = pts[3 * src];
            sorted_pts[3 * i + 1] = pts[3 * src + 1];
            sorted_pts[3 * i + 2] = pts[3 * src + 2];
        }
    }
    if (i == 0) {
        const long long n_cells = offsets[gridDim.x];
        if (n_cells >= 0 && n_cells <= N) cell_start[n_cells] = n_valid;
    }
}

// ------------------------------------------------------------------------------------------------------------ query
// first index in [lo, hi) whose key is >= key
__device__ __forceinline__ long long lower_bound(const long long* __restrict__ keys, long long lo, long long hi, long long key) {
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct Best { float d2; long long idx; };

// the points [j0, j1) of the occupied cells among x0..x1 of row (y, z): one lookup (they are consecutive in cell order); false = none
__device__ __forceinline__ bool row_range(int x0, int x1, int y, int z, const CloudGrid& g, long long n_cells, const long long* __restrict__ cell_keys,
                                          const long long* __restrict__ cell_start, long long& j0, long long& j1) {
    if (y < 0 || y >= g.ncell[1] || z < 0 || z >= g.ncell[2]) return false;
    x0 = max(x0, 0);
    x1 = min(x1, g.ncell[0] - 1);
    if (x0 > x1) return false;
    const long long a = lower_bound(cell_keys, 0, n_cells, make_key(x0, y, z));
    if (a >= n_cells) return false;
    const long long e = lower_bound(cell_keys, a, min(n_cells, a + (long long)(x1 - x0 + 1)), make_key(x1, y, z) + 1);
    if (e <= a) return false;
    j0 = cell_start[a];
    j1 = min(cell_start[e], g.n_valid);
    return true;
}

// the cells x0..x1 of row (y, z): one lookup, then their points (consecutive in cell order)
__device__ __forceinline__ void visit_row(int x0, int x1, int y, int z, const CloudGrid& g, long long n_cells, const long long* __restrict__ cell_keys,
                                          const long long* __restrict__ cell_start, const float* __restrict__ spts,
                                          const long long* __restrict__ perm, float qx, float qy, float qz, Best& best) {
    long long j0, j1;
    if (!row_range(x0, x1, y, z, g, n_cells, cell_keys, cell_start, j0, j1)) return;
    for (long long j = j0; j < j1; ++j) {
        const float dx = qx - spts[3 * j], dy = qy - spts[3 * j + 1], dz = qz - spts[3 * j + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= best.d2) {                                                // NaN never enters: the index holds finite points only
            const long long id = perm[j];
            if (d2 < best.d2 || id < best.idx || best.idx < 0) { best.d2 = d2; best.idx = id; }
        }
    }
}

__global__ __launch_bounds__(CE_THREADS) void cloud_nn_query_kernel(const float* __restrict__ q, long long M, const long long* __restrict__ q_perm,
                                                                    const CloudGrid* __restrict__ gp, const float* __restrict__ spts,
                                                                    const long long* __restrict__ perm, const long long* __restrict__ cell_keys,
                                                                    const long long* __restrict__ cell_start, float max_dist,
                                                                    float* __restrict__ dist, long long* __restrict__ idx) {
    const long long t = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (t >= M) return;
    long long qi = q_perm ? q_perm[t] : t;
    if (qi < 0 || qi >= M) return;
    const CloudGrid g = *gp;
    const float qx = q[3 * qi], qy = q[3 * qi + 1], qz = q[3 * qi + 2];
    Best best;
    best.d2 = INFINITY;
    best.idx = -1;
    const long long n_cells = g.n_cells;
    if (finite3(qx, qy, qz) && n_cells > 0) {
        const int c[3] = {query_coord(qx, g.origin[0], g.cell), query_coord(qy, g.origin[1], g.cell), query_coord(qz, g.origin[2], g.cell)};
        int s0 = 0, nmax = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            s0 = max(s0, c[a] < 0 ? -c[a] : (c[a] > g.ncell[a] - 1 ? c[a] - (g.ncell[a] - 1) : 0));        // shells below s0 hold no cell
            nmax = max(nmax, g.ncell[a]);
        }
        // see the head of the file: cells differing by s + 1 on an axis <=> farther apart than (s - slack) * cell
        const float reach = max_dist / g.cell;                              // <= MVS_CLOUD_MAX_SHELLS, checked by the host
        const int s_cap = (int)(reach * 1.0001f) + 3;                       // before slack
        const float slack = 2.4082e-7f * (float)(nmax + s_cap + 4);         // 2^-22 * 1.01
        const int s_last = s_cap + (int)slack + 1;                          // past it the bound exceeds max_dist whatever the rounding
        for (int s = s0; s <= s_last; ++s) {
            // everything not visited yet lies in shells >= s
            const float lbc = (float)(s - 1) - slack;
            if (lbc > 0.0f) {
                const float lb = lbc * g.cell * 0.99999f;
                if (lb >= max_dist || lb * lb * 0.99999f >= best.d2) break;
            }
            for (int dz = -s; dz <= s; ++dz)
                for (int dy = -s; dy <= s; ++dy) {
                    if (max(abs(dy), abs(dz)) == s) {
                        visit_row(c[0] - s, c[0] + s, c[1] + dy, c[2] + dz, g, n_cells, cell_keys, cell_start, spts, perm, qx, qy, qz, best);
                    } else {                                                // an inner row: its two end cells belong to this shell
                        visit_row(c[0] - s, c[0] - s, c[1] + dy, c[2] + dz, g, n_cells, cell_keys, cell_start, spts, perm, qx, qy, qz, best);
                        visit_row(c[0] + s, c[0] + s, c[1] + dy, c[2] + dz, g, n_cells, cell_keys, cell_start, spts, perm, qx, qy, qz, best);
                    }
                }
        }
    }
    const float d = sqrtf(best.d2);
    const bool hit = best.idx >= 0 && d < max_dist;
    dist[qi] = hit ? d : max_dist;
    idx[qi] = hit ? best.idx : -1;
}

// ------------------------------------------------------------------------------------------------------------ voxels
// one lane per occupied voxel: its points' attributes (through the permutation: original order inside the voxel) added in double
__global__ __launch_bounds__(CE_THREADS) void cloud_voxel_write_kernel(const float* __restrict__ attr, long long N, const long long* __restrict__ perm,
                                                                       const CloudGrid* __restrict__ g, const long long* __restrict__ cell_start,
                                                                       long long n_out, float* __restrict__ out) {
    const long long c = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (c >= n_out || c >= g->n_cells) return;
    const long long j0 = cell_start[c], j1 = min(cell_start[c + 1], g->n_valid);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (long long j = j0; j < j1; ++j) {
        const long long src = perm[j];
        if (src < 0 || src >= N) continue;
        sx += (double)attr[3 * src];
        sy += (double)attr[3 * src + 1];
        sz += (double)attr[3 * src + 2];
    }
    const double n = (double)(j1 - j0);
    out[3 * c] = (float)(sx / n);
    out[3 * c + 1] = (float)(sy / n);
    out[3 * c + 2] = (float)(sz / n);
}

// ------------------------------------------------------------------------------------------------------------- score
constexpr int CE_SCORE_PPT = 4, CE_SCORE_P = CE_THREADS * CE_SCORE_PPT;

__global__ __launch_bounds__(CE_THREADS) void cloud_score_kernel(const float* __restrict__ d, long long M, float max_dist, Taus taus, int K,
                                                                 CloudScore* __restrict__ rec, double* __restrict__ partial) {
    __shared__ double sred[CE_THREADS / 64];
    __shared__ uint32_t cred[1 + CE_MAXK][CE_THREADS / 64];
    const long long p0 = (long long)blockIdx.x * CE_SCORE_P + threadIdx.x;
    double s = 0.0;
    uint32_t cnt[1 + CE_MAXK];
#pragma unroll
    for (int c = 0; c <= CE_MAXK; ++c) cnt[c] = 0;
#pragma unroll
    for (int j = 0; j < CE_SCORE_PPT; ++j) {
        const long long p = p0 + (long long)j * CE_THREADS;
        const bool in = p < M;
        const float v = in ? d[p] : 0.0f;
        const bool below = in && v < max_dist;                              // a NaN distance is below nothing
        s += below ? (double)v : 0.0;
        cnt[0] += blk::ballot_count(below);
#pragma unroll
        for (int k = 0; k < CE_MAXK; ++k)
            if (k < K) cnt[1 + k] += blk::ballot_count(in && v < taus.t[k]);
    }
    blk::block_sum_put(s, sred);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c <= CE_MAXK; ++c) cred[c][threadIdx.x >> 6] = cnt[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = blk::sum4(sred);
    if (threadIdx.x <= K) {
        const uint32_t c = blk::sum4(cred[threadIdx.x]);
        long long* dst = threadIdx.x == 0 ? &rec->n_below : &rec->below_tau[threadIdx.x - 1];
        if (c) atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)c);
    }
}

// one block, after the launch above: the block sums in a fixed order, then the mean
__global__ __launch_bounds__(CE_THREADS) void cloud_score_final_kernel(const double* __restrict__ partial, long long nblk, long long M,
                                                                       CloudScore* __restrict__ rec) {
    __shared__ double sred[CE_THREADS / 64];
    double s = 0.0;
    for (long long i = threadIdx.x; i < nblk; i += CE_THREADS) s += partial[i];
    const double sum = blk::block_sum(s, sred);
    if (threadIdx.x == 0) {
        rec->n = M;
        rec->sum = sum;
        rec->mean = sum / (double)rec->n_below;                             // 0 / 0 = NaN: the mean over an empty set
    }
}

// --------------------------------------------------------------------------------------------------- greedy thinning
// DTU's rule (include/mvs_hip.h): the lexicographically first maximal independent set under the visiting order, found in rounds.  All
// per-point arrays are in CELL order (position j of the sorted index), so a neighbour scan reads consecutive points, ranks and states.
constexpr int TH_BATCH = MVS_GREEDY_THIN_BATCH;
constexpr int TH_UNDECIDED = 0, TH_KEPT = 1, TH_REMOVED = 2;

// the head of the workspace (128 bytes)
struct ThinRec {
    long long bad_order;                  // entries of `order` out of range or repeated
    long long rounds;                     // rounds that had work
    long long reserved[2];
    long long counts[TH_BATCH + 1];       // counts[i]: the length of the list round i of the current batch reads; round i adds to counts[i + 1]
    long long pad[16 - 4 - (TH_BATCH + 1)];
};
static_assert(sizeof(ThinRec) == 128, "ThinRec layout");

// inv[order[i]] = i; inv starts as all ones.  N entries into N slots: in range and never twice <=> a permutation
__global__ __launch_bounds__(CE_THREADS) void thin_rank_kernel(const long long* __restrict__ order, long long N, long long* __restrict__ inv,
                                                               ThinRec* __restrict__ rec) {
    const long long i = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (i >= N) return;
    const long long o = order[i];
    bool bad = o < 0 || o >= N;
    if (!bad) bad = atomicCAS(reinterpret_cast<unsigned long long*>(&inv[o]), ~0ull, (unsigned long long)i) != ~0ull;
    if (bad) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->bad_order), 1ull);
}

__global__ __launch_bounds__(CE_THREADS) void thin_init_kernel(const long long* __restrict__ perm, long long N, const CloudGrid* __restrict__ g,
                                                               const long long* __restrict__ inv, long long* __restrict__ srank,
                                                               int* __restrict__ sstate, long long* __restrict__ list, ThinRec* __restrict__ rec) {
    const long long j = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    const long long n_valid = min(g->n_valid, N);
    if (j == 0) rec->counts[0] = n_valid;                                   // every indexed point starts undecided
    if (j >= n_valid) return;
    const long long src = perm[j];
    srank[j] = (src >= 0 && src < N) ? inv[src] : -1;
    sstate[j] = TH_UNDECIDED;
    list[j] = j;
}

// the neighbours of point j (rank r) in the cells x0..x1 of row (y, z): true as soon as one of lower rank within dist is KEPT; `pending`
// when one of them is still UNDECIDED.  States are read with relaxed atomic loads: another block may write them during this launch, and
// any value read - old or new - is safe (a state is written once and is final).
__device__ __forceinline__ bool thin_row(int x0, int x1, int y, int z, const CloudGrid& g, long long n_cells, const long long* __restrict__ cell_keys,
                                         const long long* __restrict__ cell_start, const float* __restrict__ spts,
                                         const long long* __restrict__ srank, int* sstate, long long j, long long r, float qx, float qy,
                                         float qz, float dist2, bool& pending) {
    long long k0, k1;
    if (!row_range(x0, x1, y, z, g, n_cells, cell_keys, cell_start, k0, k1)) return false;
    for (long long k = k0; k < k1; ++k) {
        const float dx = qx - spts[3 * k], dy = qy - spts[3 * k + 1], dz = qz - spts[3 * k + 2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 <= dist2 && k != j && srank[k] < r) {
            const int s = __hip_atomic_load(&sstate[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s == TH_KEPT) return true;
            pending |= s == TH_UNDECIDED;
        }
    }
    return false;
}

// one round: lane t takes entry t of the list of undecided points; what stays undecided is appended to the next list (one 64-bit atomic
// per wavefront; the order of that list does not matter).  Blocks past the end of the list leave at once.
__global__ __launch_bounds__(CE_THREADS) void thin_round_kernel(const CloudGrid* __restrict__ gp, const float* __restrict__ spts,
                                                                const long long* __restrict__ srank, int* sstate,
                                                                const long long* __restrict__ cell_keys, const long long* __restrict__ cell_start,
                                                                float dist2, const long long* __restrict__ list_in, long long* __restrict__ list_out,
                                                                long long cap, ThinRec* rec, int round) {
    const long long n_in = min(rec->counts[round], cap);                    // written by earlier launches only
    const long long t = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    if ((long long)blockIdx.x * CE_THREADS >= n_in) return;                 // the whole block: nothing undecided here
    if (t == 0) rec->rounds += 1;
    const CloudGrid g = *gp;
    bool stay = false;
    long long j = -1;
    if (t < n_in) {
        j = list_in[t];
        if (j >= 0 && j < g.n_valid && j < cap) {
            const float qx = spts[3 * j], qy = spts[3 * j + 1], qz = spts[3 * j + 2];
            const long long r = srank[j];
            const Cell c = own_cell(qx, qy, qz, g.origin, g.cell, g.ncell);       // by the operations (and the clamp) that made its key
            bool removed = false, pending = false;
            for (int dz = -1; dz <= 1 && !removed; ++dz)
                for (int dy = -1; dy <= 1 && !removed; ++dy)
                    removed = thin_row(c.x - 1, c.x + 1, c.y + dy, c.z + dz, g, g.n_cells, cell_keys, cell_start, spts, srank, sstate, j, r, qx, qy, qz,
                                       dist2, pending);
            if (removed) __hip_atomic_store(&sstate[j], TH_REMOVED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else if (!pending) __hip_atomic_store(&sstate[j], TH_KEPT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else stay = true;
        }
    }
    const unsigned long long b = __ballot(stay);
    if (b == 0) return;                                                     // uniform over the wavefront
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)b) - 1;
    const uint32_t place = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    long long base = 0;
    if (lane == leader) base = (long long)atomicAdd(reinterpret_cast<unsigned long long*>(&rec->counts[round + 1]), (unsigned long long)__popcll(b));
    base = __shfl(base, leader, 64);
    if (stay && base + place < cap) list_out[base + place] = j;            // at most n_in <= cap entries are ever appended
}

__global__ __launch_bounds__(CE_THREADS) void thin_keep_kernel(const long long* __restrict__ perm, long long N, const CloudGrid* __restrict__ g,
                                                               const int* __restrict__ sstate, uint8_t* __restrict__ keep) {
    const long long j = (long long)blockIdx.x * CE_THREADS + threadIdx.x;
    if (j >= N || j >= g->n_valid) return;
    const long long src = perm[j];
    if (src >= 0 && src < N) keep[src] = sstate[j] == TH_KEPT ? 1 : 0;
}

}  // namespace

extern "C" int64_t mvs_greedy_thin_workspace_bytes(int64_t N) {
    if (N < 1 || N > CE_MAX_POINTS) return -1;
    return (int64_t)(sizeof(ThinRec) + 4 * 8 * N + 8 * mvs::ceil_div((long long)N, 2LL));      // record, inv / srank / two lists, states
}

extern "C" int mvs_greedy_thin(int64_t N, const int64_t* order, const void* grid, float dist, const float* sorted_pts, const int64_t* perm,
                               const int64_t* cell_keys, const int64_t* cell_start, void* workspace, uint8_t* keep, int64_t* rounds_host,
                               mvs_stream_t stream) {
    MVS_REQUIRE(order && grid && sorted_pts && perm && cell_keys && cell_start && workspace && keep && rounds_host, "mvs_greedy_thin: null pointer");
    MVS_REQUIRE(N >= 1 && N <= CE_MAX_POINTS, "mvs_greedy_thin: N=%lld points, 1..2^36 are taken (an empty cloud needs no launch)", (long long)N);
    MVS_REQUIRE(isfinite(dist) && dist > 0.0f, "mvs_greedy_thin: dist=%g must be positive and finite", (double)dist);
    MVS_REQUIRE(aligned8(order) && aligned8(grid) && aligned8(perm) && aligned8(cell_keys) && aligned8(cell_start) && aligned8(workspace),
                "mvs_greedy_thin: 64-bit arrays must be 8-byte aligned");
    hipStream_t s = MVS_STREAM(stream);
    const long long n = (long long)N;
    ThinRec* rec = reinterpret_cast<ThinRec*>(workspace);
    long long* inv = reinterpret_cast<long long*>(rec + 1);
    long long* srank = inv + n;
    long long* lists[2] = {srank + n, srank + 2 * n};
    int* sstate = reinterpret_cast<int*>(srank + 3 * n);
    const CloudGrid* g = reinterpret_cast<const CloudGrid*>(grid);
    const long long* pm = reinterpret_cast<const long long*>(perm);
    const long long* ck = reinterpret_cast<const long long*>(cell_keys);
    const long long* cs = reinterpret_cast<const long long*>(cell_start);
    const float dist2 = dist * dist;                                        // rounded once to fp32
    *rounds_host = 0;
    if (hipMemsetAsync(rec, 0, sizeof(ThinRec), s) != hipSuccess || hipMemsetAsync(inv, 0xff, 8 * (size_t)n, s) != hipSuccess ||
        hipMemsetAsync(keep, 0, (size_t)n, s) != hipSuccess)
        return mvs::finish_launch("mvs_greedy_thin(memset)");
    const unsigned nb = blocks_for(n, CE_THREADS);
    hipLaunchKernelGGL(thin_rank_kernel, dim3(nb), dim3(CE_THREADS), 0, s, reinterpret_cast<const long long*>(order), n, inv, rec);
    hipLaunchKernelGGL(thin_init_kernel, dim3(nb), dim3(CE_THREADS), 0, s, pm, n, g, inv, srank, sstate, lists[0], rec);
    if (int rc = mvs::finish_launch("mvs_greedy_thin(init)")) return rc;
    CloudGrid hg;
    ThinRec h;
    if (hipMemcpyAsync(&hg, g, sizeof(hg), hipMemcpyDeviceToHost, s) != hipSuccess || hipMemcpyAsync(&h, rec, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return mvs::finish_launch("mvs_greedy_thin(copy)");
    MVS_REQUIRE(h.bad_order == 0, "mvs_greedy_thin: order is not a permutation of 0..%lld (%lld entries out of range or repeated)", n - 1, h.bad_order);
    MVS_REQUIRE(hg.n_valid >= 0 && hg.n_valid <= n && hg.n_cells >= 0 && hg.n_cells <= hg.n_valid, "mvs_greedy_thin: the grid does not belong to %lld points", n);
    const float slack = 2.4082e-7f * (float)(std::max(hg.ncell[0], std::max(hg.ncell[1], hg.ncell[2])) + 4);     // 2^-22 * 1.01, as in the query
    MVS_REQUIRE(0.99999f * (1.0f - slack) * hg.cell >= dist, "mvs_greedy_thin: cell=%g is too small for dist=%g: neighbours must lie in adjacent cells",
                (double)hg.cell, (double)dist);
    long long cur = h.counts[0];
    int side = 0;
    while (cur > 0) {
        MVS_REQUIRE(h.rounds <= n, "mvs_greedy_thin: %lld points still undecided after %lld rounds", cur, h.rounds);
        if (hipMemsetAsync(&rec->counts[1], 0, 8 * TH_BATCH, s) != hipSuccess) return mvs::finish_launch("mvs_greedy_thin(memset)");
        for (int i = 0; i < TH_BATCH; ++i, side ^= 1)                      // counts only fall: `cur` bounds every list of the batch
            hipLaunchKernelGGL(thin_round_kernel, dim3(blocks_for(cur, CE_THREADS)), dim3(CE_THREADS), 0, s, g, sorted_pts, srank, sstate, ck, cs, dist2,
                               lists[side], lists[side ^ 1], n, rec, i);
        if (int rc = mvs::finish_launch("mvs_greedy_thin(round)")) return rc;
        if (hipMemcpyAsync(&rec->counts[0], &rec->counts[TH_BATCH], 8, hipMemcpyDeviceToDevice, s) != hipSuccess ||
            hipMemcpyAsync(&h, rec, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
            return mvs::finish_launch("mvs_greedy_thin(copy)");
        cur = h.counts[0];
    }
    hipLaunchKernelGGL(thin_keep_kernel, dim3(nb), dim3(CE_THREADS), 0, s, pm, n, g, sstate, keep);
    *rounds_host = h.rounds;
    return mvs::finish_launch("mvs_greedy_thin");
}

extern "C" int mvs_cloud_bounds(const float* pts, int64_t N, void* grid, float* bounds_host, int64_t* n_nonfinite_host, mvs_stream_t stream) {
    MVS_REQUIRE(pts && grid && bounds_host && n_nonfinite_host, "mvs_cloud_bounds: null pointer");
    MVS_REQUIRE(N >= 1 && N <= CE_MAX_POINTS, "mvs_cloud_bounds: N=%lld points, 1..2^36 are taken (an empty cloud needs no launch)", (long long)N);
    MVS_REQUIRE(aligned8(grid), "mvs_cloud_bounds: the grid record must be 8-byte aligned");
    hipStream_t s = MVS_STREAM(stream);
    CloudGrid* g = reinterpret_cast<CloudGrid*>(grid);
    if (hipMemsetAsync(g, 0, MVS_CLOUD_GRID_RECORD_BYTES, s) != hipSuccess || hipMemsetAsync(g->lo_bits, 0xff, sizeof(g->lo_bits), s) != hipSuccess)
        return mvs::finish_launch("mvs_cloud_bounds(memset)");
    const unsigned nb = (unsigned)std::min<long long>(mvs::ceil_div((long long)N, (long long)CE_THREADS), 4096);
    hipLaunchKernelGGL(cloud_bounds_kernel, dim3(nb), dim3(CE_THREADS), 0, s, pts, (long long)N, g);
    if (int rc = mvs::finish_launch("mvs_cloud_bounds")) return rc;
    CloudGrid h;
    if (hipMemcpyAsync(&h, g, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return mvs::finish_launch("mvs_cloud_bounds(copy)");
    const bool none = h.n_bad >= N;
    for (int a = 0; a < 3; ++a) {
        bounds_host[a] = none ? 0.0f : from_order_bits(h.lo_bits[a]);
        bounds_host[3 + a] = none ? 0.0f : from_order_bits(h.hi_bits[a]);
    }
    *n_nonfinite_host = h.n_bad;
    return MVS_OK;
}

extern "C" int mvs_cloud_grid_keys(const float* pts, int64_t N, float cell, const float* bounds_host, int64_t n_nonfinite, void* grid,
                                   int64_t* keys, mvs_stream_t stream) {
    MVS_REQUIRE(pts && bounds_host && grid && keys, "mvs_cloud_grid_keys: null pointer");
    MVS_REQUIRE(N >= 1 && N <= CE_MAX_POINTS && n_nonfinite >= 0 && n_nonfinite <= N, "mvs_cloud_grid_keys: N=%lld points (%lld non-finite)",
                (long long)N, (long long)n_nonfinite);
    MVS_REQUIRE(isfinite(cell) && cell > 0.0f, "mvs_cloud_grid_keys: cell=%g must be positive and finite", (double)cell);
    MVS_REQUIRE(aligned8(grid) && aligned8(keys), "mvs_cloud_grid_keys: the grid record and the keys must be 8-byte aligned");
    GridSetup gs;
    gs.cell = cell;
    gs.n_valid = N - n_nonfinite;
    for (int a = 0; a < 3; ++a) {
        const float lo = bounds_host[a], hi = bounds_host[3 + a];
        MVS_REQUIRE(isfinite(lo) && isfinite(hi) && lo <= hi, "mvs_cloud_grid_keys: bad bounds [%g, %g] on axis %d", (double)lo, (double)hi, a);
        const float top = cell_coord(hi, lo, cell);                         // the largest cell coordinate any point of the cloud gets
        MVS_REQUIRE(top < (float)CE_AXIS_CELLS, "mvs_cloud_grid_keys: axis %d spans %g cells of %g, fewer than 2^21 are indexed", a,
                    (double)top + 1.0, (double)cell);
        gs.origin[a] = lo;
        gs.ncell[a] = (int)top + 1;
    }
    hipLaunchKernelGGL(cloud_keys_kernel, dim3(blocks_for(N, CE_THREADS)), dim3(CE_THREADS), 0, MVS_STREAM(stream), pts, (long long)N, gs,
                       reinterpret_cast<CloudGrid*>(grid), reinterpret_cast<long long*>(keys));
    return mvs::finish_launch("mvs_cloud_grid_keys");
}

extern "C" int mvs_cloud_query_keys(const float* queries, int64_t M, const void* grid, int64_t* keys, mvs_stream_t stream) {
    MVS_REQUIRE(queries && grid && keys, "mvs_cloud_query_keys: null pointer");
    MVS_REQUIRE(M >= 1 && M <= CE_MAX_POINTS, "mvs_cloud_query_keys: M=%lld queries, 1..2^36 are taken", (long long)M);
    MVS_REQUIRE(aligned8(grid) && aligned8(keys), "mvs_cloud_query_keys: the grid record and the keys must be 8-byte aligned");
    hipLaunchKernelGGL(cloud_query_keys_kernel, dim3(blocks_for(M, CE_THREADS)), dim3(CE_THREADS), 0, MVS_STREAM(stream), queries, (long long)M,
                       reinterpret_cast<const CloudGrid*>(grid), reinterpret_cast<long long*>(keys));
    return mvs::finish_launch("mvs_cloud_query_keys");
}

extern "C" int64_t mvs_cloud_grid_workspace_bytes(int64_t N) {
    if (N < 1 || N > CE_MAX_POINTS) return -1;
    const long long nb = mvs::ceil_div((long long)N, (long long)CE_THREADS);
    return (int64_t)((nb + 1) * 8 + nb * 4);
}

extern "C" int mvs_cloud_grid_build(const float* pts, int64_t N, const int64_t* sorted_keys, const int64_t* perm, void* grid, void* workspace,
                                    float* sorted_pts, int64_t* cell_keys, int64_t* cell_start, mvs_stream_t stream) {
    MVS_REQUIRE(pts && sorted_keys && perm && grid && workspace && cell_keys && cell_start, "mvs_cloud_grid_build: null pointer");
    MVS_REQUIRE(N >= 1 && N <= CE_MAX_POINTS, "mvs_cloud_grid_build: N=%lld points, 1..2^36 are taken", (long long)N);
    MVS_REQUIRE(aligned8(grid) && aligned8(workspace) && aligned8(sorted_keys) && aligned8(perm) && aligned8(cell_keys) && aligned8(cell_start),
                "mvs_cloud_grid_build: 64-bit arrays must be 8-byte aligned");
    hipStream_t s = MVS_STREAM(stream);
    const long long nb = mvs::ceil_div((long long)N, (long long)CE_THREADS);
    long long* offsets = reinterpret_cast<long long*>(workspace);
    uint32_t* counts = reinterpret_cast<uint32_t*>(offsets + nb + 1);
    CloudGrid* g = reinterpret_cast<CloudGrid*>(grid);
    const long long* sk = reinterpret_cast<const long long*>(sorted_keys);
    const long long* pm = reinterpret_cast<const long long*>(perm);
    hipLaunchKernelGGL(cloud_heads_count_kernel, dim3((unsigned)nb), dim3(CE_THREADS), 0, s, sk, (long long)N, g, counts);
    blk::launch_exclusive_scan_u32(counts, nb, offsets, &g->n_cells, s);
    hipLaunchKernelGGL(cloud_build_kernel, dim3((unsigned)nb), dim3(CE_THREADS), 0, s, pts, (long long)N, sk, pm, g, offsets, sorted_pts,
                       reinterpret_cast<long long*>(cell_keys), reinterpret_cast<long long*>(cell_start));
    return mvs::finish_launch("mvs_cloud_grid_build");
}

extern "C" int mvs_cloud_nn_query(const float* queries, int64_t M, const int64_t* query_perm, const void* grid, float cell, const float* sorted_pts,
                                  const int64_t* perm, const int64_t* cell_keys, const int64_t* cell_start, int64_t N, float max_dist, float* dist,
                                  int64_t* idx, mvs_stream_t stream) {
    MVS_REQUIRE(queries && grid && sorted_pts && perm && cell_keys && cell_start && dist && idx, "mvs_cloud_nn_query: null pointer");
    MVS_REQUIRE(M >= 1 && M <= CE_MAX_POINTS && N >= 1 && N <= CE_MAX_POINTS,
                "mvs_cloud_nn_query: M=%lld queries, N=%lld targets (an empty side needs no launch)", (long long)M, (long long)N);
    MVS_REQUIRE(isfinite(cell) && cell > 0.0f && isfinite(max_dist) && max_dist > 0.0f, "mvs_cloud_nn_query: cell=%g and max_dist=%g must be positive and finite",
                (double)cell, (double)max_dist);
    MVS_REQUIRE(max_dist / cell <= (float)MVS_CLOUD_MAX_SHELLS, "mvs_cloud_nn_query: max_dist / cell = %g, at most %d shells are walked",
                (double)(max_dist / cell), MVS_CLOUD_MAX_SHELLS);
    MVS_REQUIRE(aligned8(grid) && aligned8(query_perm) && aligned8(perm) && aligned8(cell_keys) && aligned8(cell_start) && aligned8(idx),
                "mvs_cloud_nn_query: 64-bit arrays must be 8-byte aligned");
    hipLaunchKernelGGL(cloud_nn_query_kernel, dim3(blocks_for(M, CE_THREADS)), dim3(CE_THREADS), 0, MVS_STREAM(stream), queries, (long long)M,
                       reinterpret_cast<const long long*>(query_perm), reinterpret_cast<const CloudGrid*>(grid), sorted_pts,
                       reinterpret_cast<const long long*>(perm), reinterpret_cast<const long long*>(cell_keys),
                       reinterpret_cast<const long long*>(cell_start), max_dist, dist, reinterpret_cast<long long*>(idx));
    return mvs::finish_launch("mvs_cloud_nn_query");
}

extern "C" int mvs_cloud_voxel_downsample_count(const void* grid, int64_t* count_host, mvs_stream_t stream) {
    MVS_REQUIRE(grid && count_host, "mvs_cloud_voxel_downsample_count: null pointer");
    hipStream_t s = MVS_STREAM(stream);
    CloudGrid h;
    if (hipMemcpyAsync(&h, grid, sizeof(h), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return mvs::finish_launch("mvs_cloud_voxel_downsample_count(copy)");
    *count_host = h.n_cells;
    return MVS_OK;
}

extern "C" int mvs_cloud_voxel_downsample_write(const float* attr, int64_t N, const int64_t* perm, const void* grid, const int64_t* cell_start,
                                                int64_t count, float* out, mvs_stream_t stream) {
    MVS_REQUIRE(attr && perm && grid && cell_start && out, "mvs_cloud_voxel_downsample_write: null pointer");
    MVS_REQUIRE(N >= 1 && N <= CE_MAX_POINTS && count >= 1 && count <= N,
                "mvs_cloud_voxel_downsample_write: N=%lld points, count=%lld voxels (an empty cloud needs no launch)", (long long)N, (long long)count);
    MVS_REQUIRE(aligned8(grid) && aligned8(perm) && aligned8(cell_start), "mvs_cloud_voxel_downsample_write: 64-bit arrays must be 8-byte aligned");
    hipLaunchKernelGGL(cloud_voxel_write_kernel, dim3(blocks_for(count, CE_THREADS)), dim3(CE_THREADS), 0, MVS_STREAM(stream), attr, (long long)N,
                       reinterpret_cast<const long long*>(perm), reinterpret_cast<const CloudGrid*>(grid),
                       reinterpret_cast<const long long*>(cell_start), (long long)count, out);
    return mvs::finish_launch("mvs_cloud_voxel_downsample_write");
}

extern "C" int64_t mvs_cloud_score_workspace_bytes(int64_t M) {
    if (M < 0 || M > CE_MAX_POINTS) return -1;
    return (int64_t)(8 * std::max<long long>(1, mvs::ceil_div((long long)M, (long long)CE_SCORE_P)));
}

extern "C" int mvs_cloud_score(const float* dist, int64_t M, float max_dist, const float* taus_host, int K, void* workspace, void* record,
                               mvs_stream_t stream) {
    MVS_REQUIRE(record && workspace && (M == 0 || dist) && (K == 0 || taus_host), "mvs_cloud_score: null pointer");
    MVS_REQUIRE(M >= 0 && M <= CE_MAX_POINTS, "mvs_cloud_score: M=%lld distances", (long long)M);
    MVS_REQUIRE(K >= 0 && K <= CE_MAXK, "mvs_cloud_score: K=%d thresholds, 0..%d are built", K, CE_MAXK);
    MVS_REQUIRE(isfinite(max_dist) && max_dist > 0.0f, "mvs_cloud_score: max_dist=%g must be positive and finite", (double)max_dist);
    MVS_REQUIRE(aligned8(record) && aligned8(workspace), "mvs_cloud_score: the record and the workspace must be 8-byte aligned");
    Taus taus;
    for (int k = 0; k < CE_MAXK; ++k) taus.t[k] = 0.0f;
    for (int k = 0; k < K; ++k) {
        MVS_REQUIRE(taus_host[k] <= max_dist, "mvs_cloud_score: tau[%d]=%g exceeds max_dist=%g", k, (double)taus_host[k], (double)max_dist);   // NaN fails too
        taus.t[k] = taus_host[k];
    }
    hipStream_t s = MVS_STREAM(stream);
    CloudScore* rec = reinterpret_cast<CloudScore*>(record);
    if (hipMemsetAsync(rec, 0, sizeof(CloudScore), s) != hipSuccess) return mvs::finish_launch("mvs_cloud_score(memset)");
    const long long nblk = mvs::ceil_div((long long)M, (long long)CE_SCORE_P);
    double* partial = reinterpret_cast<double*>(workspace);
    if (nblk > 0) hipLaunchKernelGGL(cloud_score_kernel, dim3((unsigned)nblk), dim3(CE_THREADS), 0, s, dist, (long long)M, max_dist, taus, K, rec, partial);
    hipLaunchKernelGGL(cloud_score_final_kernel, dim3(1), dim3(CE_THREADS), 0, s, partial, nblk, (long long)M, rec);
    return mvs::finish_launch("mvs_cloud_score");
}
