// Flash attention for the DINO ViT in training mode ("fix": false; models/vision_transformer.py:139-150 under autograd): the forward with the
// row log-sum-exp and a deterministic two-pass backward.  No N x N tensor exists anywhere: the forward keeps out [B][N][C] and lse [B][heads][N],
// the backward recomputes P = exp(scale * S - lse) tile by tile.  Same arithmetic as csrc/vit.hip / csrc/vit_packed.hip: every matrix product
// on the bf16 matrix cores in the three-term split form of split3.h (six v_mfma_f32_16x16x32_bf16 per K = 32 step, fp32 accumulation) -
// fp32-equivalent.  head dimension 64 only.  qkv = [B][N][3C] packed rows (q | k | v, head h at columns h * 64), C = heads * 64.
//
//   flash_train_fwd_kernel    block = 64 queries (4 wavefronts x 16), loop over tiles of 32 keys.  S^T [key][query] = K Q^T (csrc/vit_packed.hip's
//                             orientation): a lane's eight accumulators are the scores of ONE query against keys pi(kb, e) - online softmax with
//                             per-lane scalars, and the eight P values, split in registers, ARE the second operand of O^T += V^T P^T.
//   flash_train_cls_kernel    P_0 = exp(scale * q_0 . k - lse_0): the CLS query's row [B][heads][N] (the only attention values the model reads)
//   flash_train_delta_kernel  D[b][h][i] = sum_c dO . O (the row sums of P * dP);  flash_train_cls_delta_kernel adds sum_k P_0k dA_0k to D_0 -
//                             with g = dP + dA the softmax backward of row 0 is scale * P * (g - sum P g)
//   flash_train_dkv_kernel    block = 64 keys, loop over tiles of 32 queries.  S [query][key] = Q K^T, dP = dO V^T: a lane holds eight queries of
//                             ONE key; P and dS = scale * P * (dP - D) are split in registers and are the second operands of
//                             dV^T += dO^T P and dK^T += Q^T dS (accumulated in registers over all query tiles)
//   flash_train_dq_kernel     block = 64 queries, loop over tiles of 32 keys, the forward's orientation: dQ^T += K^T dS^T
// Each output element is owned by one lane and summed in a fixed order: no atomics, two runs are bitwise equal.
//
// LDS tiles of 32 tokens x 64 d, three bf16 terms each: "row-major" [token][d] (128-byte rows; operands contracted over d) and "transposed"
// [d][token] (64-byte rows; operands contracted over tokens), the tokens of a transposed row stored in the order pi - token 16 nt + 4 kb + r at
// position 8 kb + 4 nt + r - so that chunk kb of a row is exactly the eight tokens a lane of group kb holds accumulators for.  16-byte chunks
// are xor-swizzled against bank conflicts as in csrc/vit.hip.
#include "common.h"
#include "prims.h"
#include "split3.h"

namespace {
using mvsx3::bf16x8;
using mvsx3::Split3;
using mvsprim::f32x4;

constexpr int FT_TOK = 32;                                   // tokens per LDS tile
constexpr int FT_RTERM = FT_TOK * 128, FT_TTERM = 64 * 64;   // bytes of one term of a row-major / transposed tile
constexpr int FT_RTILE = 3 * FT_RTERM, FT_TTILE = 3 * FT_TTERM;
constexpr float FT_LOG2E = 1.4426950408889634f, FT_LN2 = 0.6931471805599453f;

__device__ __forceinline__ int roff(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
__device__ __forceinline__ int toff(int d, int chunk) { return d * 64 + ((chunk ^ ((d >> 2) & 3)) << 4); }

struct Row8 { f32x4 lo, hi; };

// 8 consecutive d of token `row` (zeros beyond N); base = the (image, head)'s first element, rows ld floats apart, 16-byte aligned
__device__ __forceinline__ Row8 load_row8(const float* __restrict__ base, size_t ld, int row, int N, int d0) {
    Row8 v;
    v.lo = v.hi = f32x4{0.f, 0.f, 0.f, 0.f};
    if (row < N) {
        const float* p = base + (size_t)row * ld + d0;
        v.lo = *reinterpret_cast<const f32x4*>(p), v.hi = *reinterpret_cast<const f32x4*>(p + 4);
    }
    return v;
}

__device__ __forceinline__ Split3 split_row(const Row8& r) {
    const float v[8] = {r.lo[0], r.lo[1], r.lo[2], r.lo[3], r.hi[0], r.hi[1], r.hi[2], r.hi[3]};
    return mvsx3::split3(v);
}

// staging: thread (row = tid / 8, 8 d at (tid % 8) * 8) of a 32 x 64 tile
__device__ __forceinline__ void put_rm(unsigned char* tile, int row, int dseg, const Split3& s) {
    unsigned char* d = tile + roff(row, dseg);
    *reinterpret_cast<bf16x8*>(d) = s.h;
    *reinterpret_cast<bf16x8*>(d + FT_RTERM) = s.m;
    *reinterpret_cast<bf16x8*>(d + 2 * FT_RTERM) = s.l;
}
__device__ __forceinline__ void put_tr(unsigned char* tile, int row, int dseg, const Split3& s) {
    const int pos = ((row >> 2) & 3) * 8 + (row >> 4) * 4 + (row & 3);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        unsigned char* d = tile + toff(dseg * 8 + e, pos >> 3) + (pos & 7) * 2;
        *reinterpret_cast<__bf16*>(d) = s.h[e];
        *reinterpret_cast<__bf16*>(d + FT_TTERM) = s.m[e];
        *reinterpret_cast<__bf16*>(d + 2 * FT_TTERM) = s.l[e];
    }
}

struct Frag { bf16x8 h, m, l; };
// first-operand fragments: row-major tile, lane (i = token `row`, kb) holds d = 32 st + 8 kb .. + 7; transposed tile, lane (i = d, kb)
// holds tokens pi(kb, 0..7)
__device__ __forceinline__ Frag rm_frag(const unsigned char* tile, int row, int st, int kb) {
    const unsigned char* p = tile + roff(row, 4 * st + kb);
    return Frag{*reinterpret_cast<const bf16x8*>(p), *reinterpret_cast<const bf16x8*>(p + FT_RTERM), *reinterpret_cast<const bf16x8*>(p + 2 * FT_RTERM)};
}
__device__ __forceinline__ Frag tr_frag(const unsigned char* tile, int d, int kb) {
    const unsigned char* p = tile + toff(d, kb);
    return Frag{*reinterpret_cast<const bf16x8*>(p), *reinterpret_cast<const bf16x8*>(p + FT_TTERM), *reinterpret_cast<const bf16x8*>(p + 2 * FT_TTERM)};
}
__device__ __forceinline__ Frag split_frag(const float (&v)[8]) {
    const Split3 s = mvsx3::split3(v);
    return Frag{s.h, s.m, s.l};
}
__device__ __forceinline__ f32x4 mma(const Frag& a, const Frag& b, f32x4 c) { return mvsx3::mfma6(a.h, a.m, a.l, b.h, b.m, b.l, c); }

// second-operand fragments of the wavefront's own 16 tokens, straight from memory: lane (j = token, kb) holds d = 32 st + 8 kb .. + 7
__device__ __forceinline__ void own_frags(const float* __restrict__ base, size_t ld, int row, int N, int kb, Frag (&f)[2]) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        const Split3 s = split_row(load_row8(base, ld, row, N, 32 * st + 8 * kb));
        f[st] = Frag{s.h, s.m, s.l};
    }
}

// ---------------------------------------------------------------------------------------------------------------- forward
__global__ __launch_bounds__(256, 2) void flash_train_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse, int N,
                                                                 int NH, float scale2) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[FT_RTILE + FT_TTILE];
    unsigned char* kl = lds;                                 // K row-major
    unsigned char* vl = lds + FT_RTILE;                      // V transposed
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kb = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z, C = NH * 64;
    const size_t ld = (size_t)3 * C;
    const float* qb = qkv + (size_t)b * N * ld + h * 64;
    const int myq = blockIdx.x * 64 + wave * 16 + j;
    Frag qf[2];
    own_frags(qb, ld, myq, N, kb, qf);
    f32x4 o[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float mrow = -INFINITY, lrow = 0.0f;                     // base-2 running maximum (shared by the query's four lanes), this lane's partial sum
    const int srow = tid >> 3, sseg = tid & 7;
    Row8 pk, pv;
    auto fetch = [&](int kt) {
        pk = load_row8(qb + C, ld, kt + srow, N, sseg * 8);
        pv = load_row8(qb + 2 * C, ld, kt + srow, N, sseg * 8);
    };
    fetch(0);
    for (int kt = 0; kt < N; kt += FT_TOK) {
        __syncthreads();                                     // the previous tile's fragments are consumed
        put_rm(kl, srow, sseg, split_row(pk));
        put_tr(vl, srow, sseg, split_row(pv));
        __syncthreads();
        if (kt + FT_TOK < N) fetch(kt + FT_TOK);
        float p[8];
        float lmax = -INFINITY;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < 2; ++st) c = mma(rm_frag(kl, nt * 16 + j, st, kb), qf[st], c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float s = kt + nt * 16 + 4 * kb + r < N ? c[r] * scale2 : -INFINITY;
                p[4 * nt + r] = s;
                lmax = fmaxf(lmax, s);
            }
        }
        lmax = fmaxf(lmax, __shfl_xor(lmax, 16, 64));
        lmax = fmaxf(lmax, __shfl_xor(lmax, 32, 64));        // finite: key kt of the tile is < N
        const float mnew = fmaxf(mrow, lmax);
        const float alpha = __builtin_amdgcn_exp2f(mrow - mnew);             // 0 at the first tile
        mrow = mnew;
        float sum = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            p[e] = __builtin_amdgcn_exp2f(p[e] - mnew);
            sum += p[e];
        }
        lrow = lrow * alpha + sum;
        const Frag pf = split_frag(p);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            o[t] *= alpha;
            o[t] = mma(tr_frag(vl, t * 16 + j, kb), pf, o[t]);
        }
    }
    lrow += __shfl_xor(lrow, 16, 64);
    lrow += __shfl_xor(lrow, 32, 64);
    if (myq >= N) return;
    const float inv = 1.0f / lrow;
    float* op = out + ((size_t)b * N + myq) * C + h * 64 + 4 * kb;           // o[t][r] = O[query j][d = 16 t + 4 kb + r]
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(op + 16 * t) = o[t] * inv;
    if (kb == 0) lse[((size_t)b * NH + h) * N + myq] = (mrow + log2f(lrow)) * FT_LN2;
}

// ---------------------------------------------------------------------------------------------------------------- CLS row
// p[key] = exp(scale * q_0 . k_key - lse_0) per (image, head), fp32 FMA chains; dA given: returns through `delta0` D_0 += sum_k p_k dA_k instead
// (block-wide sum in a fixed order)
__global__ __launch_bounds__(256) void flash_train_cls_kernel(const float* __restrict__ qkv, const float* __restrict__ lse, float* __restrict__ att,
                                                              const float* __restrict__ dA, float* __restrict__ delta0, int N, int NH, float scale2) {
    __shared__ float q[64];
    __shared__ float red[4];
    const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, C = NH * 64;
    const size_t ld = (size_t)3 * C, bh = (size_t)b * NH + h;
    const float* qb = qkv + (size_t)b * N * ld + h * 64;
    if (tid < 64) q[tid] = qb[tid];
    __syncthreads();
    const float l2 = lse[bh * N] * FT_LOG2E;
    float sum = 0.0f;
    for (int key = tid; key < N; key += 256) {
        const float* kp = qb + C + (size_t)key * ld;
        float acc = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kp + 4 * c);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = fmaf(q[4 * c + e], kv[e], acc);
        }
        const float p = __builtin_amdgcn_exp2f(acc * scale2 - l2);
        if (att) att[bh * N + key] = p;
        if (dA) sum = fmaf(p, dA[bh * N + key], sum);
    }
    if (!dA) return;                                         // (uniform)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) delta0[bh * N] += (red[0] + red[1]) + (red[2] + red[3]);
}

// ---------------------------------------------------------------------------------------------------------------- D = rowsum(dO * O)
__global__ __launch_bounds__(256) void flash_train_delta_kernel(const float* __restrict__ out, const float* __restrict__ dout, float* __restrict__ delta,
                                                                int N, int NH) {
    const int h = blockIdx.y, b = blockIdx.z, C = NH * 64;
    const int row = blockIdx.x * 16 + (threadIdx.x >> 4), sub = threadIdx.x & 15;
    float s = 0.0f;
    if (row < N) {
        const size_t o = ((size_t)b * N + row) * C + h * 64 + 4 * sub;
        const f32x4 a = *reinterpret_cast<const f32x4*>(out + o), d = *reinterpret_cast<const f32x4*>(dout + o);
        s = fmaf(a[0], d[0], fmaf(a[1], d[1], fmaf(a[2], d[2], a[3] * d[3])));
    }
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (sub == 0 && row < N) delta[((size_t)b * NH + h) * N + row] = s;
}

// ---------------------------------------------------------------------------------------------------------------- dK, dV
__global__ __launch_bounds__(256, 2) void flash_train_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                                                                 const float* __restrict__ delta, const float* __restrict__ dA, float* __restrict__ dqkv,
                                                                 int N, int NH, float scale, float scale2) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * FT_RTILE + 2 * FT_TTILE];
    __shared__ __attribute__((aligned(16))) float rowv[2][FT_TOK];           // lse * log2(e) (+inf beyond N) | D of the tile's queries
    unsigned char* ql = lds;                                 // Q, dO row-major; Q, dO transposed
    unsigned char* dl = lds + FT_RTILE;
    unsigned char* qt = lds + 2 * FT_RTILE;
    unsigned char* dt = lds + 2 * FT_RTILE + FT_TTILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kb = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z, C = NH * 64;
    const size_t ld = (size_t)3 * C, bh = (size_t)b * NH + h;
    const float* qb = qkv + (size_t)b * N * ld + h * 64;
    const float* dob = dout + (size_t)b * N * C + h * 64;
    const int mykey = blockIdx.x * 64 + wave * 16 + j;
    Frag kf[2], vf[2];
    own_frags(qb + C, ld, mykey, N, kb, kf);
    own_frags(qb + 2 * C, ld, mykey, N, kb, vf);
    const float da0 = dA && mykey < N ? dA[bh * N + mykey] : 0.0f;           // the CLS query's dA at this lane's key
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dk[t] = dv[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int srow = tid >> 3, sseg = tid & 7;
    Row8 pq, pd;
    float prow = 0.0f;
    auto fetch = [&](int q0) {
        pq = load_row8(qb, ld, q0 + srow, N, sseg * 8);
        pd = load_row8(dob, (size_t)C, q0 + srow, N, sseg * 8);
        if (tid < FT_TOK) prow = q0 + tid < N ? lse[bh * N + q0 + tid] * FT_LOG2E : INFINITY;
        else if (tid < 2 * FT_TOK) prow = q0 + tid - FT_TOK < N ? delta[bh * N + q0 + tid - FT_TOK] : 0.0f;
    };
    fetch(0);
    for (int q0 = 0; q0 < N; q0 += FT_TOK) {
        __syncthreads();
        {
            const Split3 sq = split_row(pq), sd = split_row(pd);
            put_rm(ql, srow, sseg, sq);
            put_tr(qt, srow, sseg, sq);
            put_rm(dl, srow, sseg, sd);
            put_tr(dt, srow, sseg, sd);
            if (tid < 2 * FT_TOK) rowv[tid >> 5][tid & 31] = prow;
        }
        __syncthreads();
        if (q0 + FT_TOK < N) fetch(q0 + FT_TOK);
        float p[8], ds[8];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                s = mma(rm_frag(ql, nt * 16 + j, st, kb), kf[st], s);        // S [query 16 nt + 4 kb + r][key j]
                g = mma(rm_frag(dl, nt * 16 + j, st, kb), vf[st], g);        // dP
            }
            const f32x4 l2 = *reinterpret_cast<const f32x4*>(&rowv[0][nt * 16 + 4 * kb]);
            const f32x4 dd = *reinterpret_cast<const f32x4*>(&rowv[1][nt * 16 + 4 * kb]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pv = mykey < N ? __builtin_amdgcn_exp2f(s[r] * scale2 - l2[r]) : 0.0f;          // 0 for queries beyond N (l2 = +inf)
                float gg = g[r];
                if (q0 + nt * 16 + 4 * kb + r == 0) gg += da0;
                p[4 * nt + r] = pv;
                ds[4 * nt + r] = scale * pv * (gg - dd[r]);
            }
        }
        const Frag pf = split_frag(p), sf = split_frag(ds);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            dv[t] = mma(tr_frag(dt, t * 16 + j, kb), pf, dv[t]);             // dV^T [d][key] += dO^T P
            dk[t] = mma(tr_frag(qt, t * 16 + j, kb), sf, dk[t]);             // dK^T [d][key] += Q^T dS
        }
    }
    if (mykey >= N) return;
    float* kp = dqkv + ((size_t)b * N + mykey) * ld + C + h * 64 + 4 * kb;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        *reinterpret_cast<f32x4*>(kp + 16 * t) = dk[t];
        *reinterpret_cast<f32x4*>(kp + C + 16 * t) = dv[t];
    }
}

// ---------------------------------------------------------------------------------------------------------------- dQ
__global__ __launch_bounds__(256, 2) void flash_train_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ dout, const float* __restrict__ lse,
                                                                const float* __restrict__ delta, const float* __restrict__ dA, float* __restrict__ dqkv,
                                                                int N, int NH, float scale, float scale2) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * FT_RTILE + FT_TTILE];
    unsigned char* kl = lds;                                 // K, V row-major; K transposed
    unsigned char* vl = lds + FT_RTILE;
    unsigned char* kt_ = lds + 2 * FT_RTILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 15, kb = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z, C = NH * 64;
    const size_t ld = (size_t)3 * C, bh = (size_t)b * NH + h;
    const float* qb = qkv + (size_t)b * N * ld + h * 64;
    const int myq = blockIdx.x * 64 + wave * 16 + j;
    Frag qf[2], df[2];
    own_frags(qb, ld, myq, N, kb, qf);
    own_frags(dout + (size_t)b * N * C + h * 64, (size_t)C, myq, N, kb, df);
    const float l2 = myq < N ? lse[bh * N + myq] * FT_LOG2E : INFINITY;
    const float dd = myq < N ? delta[bh * N + myq] : 0.0f;
    const float* darow = dA && myq == 0 ? dA + bh * N : nullptr;
    f32x4 dq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) dq[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int srow = tid >> 3, sseg = tid & 7;
    Row8 pk, pv;
    auto fetch = [&](int kt) {
        pk = load_row8(qb + C, ld, kt + srow, N, sseg * 8);
        pv = load_row8(qb + 2 * C, ld, kt + srow, N, sseg * 8);
    };
    fetch(0);
    for (int kt = 0; kt < N; kt += FT_TOK) {
        __syncthreads();
        {
            const Split3 sk = split_row(pk);
            put_rm(kl, srow, sseg, sk);
            put_tr(kt_, srow, sseg, sk);
            put_rm(vl, srow, sseg, split_row(pv));
        }
        __syncthreads();
        if (kt + FT_TOK < N) fetch(kt + FT_TOK);
        float ds[8];
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                s = mma(rm_frag(kl, nt * 16 + j, st, kb), qf[st], s);        // S^T [key 16 nt + 4 kb + r][query j]
                g = mma(rm_frag(vl, nt * 16 + j, st, kb), df[st], g);        // dP^T
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kt + nt * 16 + 4 * kb + r;
                const float p = key < N ? __builtin_amdgcn_exp2f(s[r] * scale2 - l2) : 0.0f;              // 0 for queries beyond N (l2 = +inf)
                float gg = g[r];
                if (darow && key < N) gg += darow[key];
                ds[4 * nt + r] = scale * p * (gg - dd);
            }
        }
        const Frag sf = split_frag(ds);
#pragma unroll
        for (int t = 0; t < 4; ++t) dq[t] = mma(tr_frag(kt_, t * 16 + j, kb), sf, dq[t]);                  // dQ^T [d][query] += K^T dS^T
    }
    if (myq >= N) return;
    float* qp = dqkv + ((size_t)b * N + myq) * ld + h * 64 + 4 * kb;
#pragma unroll
    for (int t = 0; t < 4; ++t) *reinterpret_cast<f32x4*>(qp + 16 * t) = dq[t];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int mvs_attention_train_fwd_flash(const float* qkv, float* out, float* lse, float* cls_row, int B, int N, int heads, int head_dim,
                                             float scale, mvs_stream_t stream) {
    MVS_REQUIRE(qkv && out && lse && B >= 1 && B <= 65535 && N >= 1 && heads >= 1 && heads <= 65535, "mvs_attention_train_fwd_flash: bad shape");
    MVS_REQUIRE(head_dim == 64, "mvs_attention_train_fwd_flash: head dimension 64 only (got %d)", head_dim);
    MVS_REQUIRE(aligned16(qkv) && aligned16(out), "mvs_attention_train_fwd_flash: qkv and out must be 16-byte aligned");
    MVS_REQUIRE((int64_t)N + 63 < ((int64_t)1 << 31), "mvs_attention_train_fwd_flash: N too large");
    const float scale2 = scale * FT_LOG2E;
    hipLaunchKernelGGL(flash_train_fwd_kernel, dim3((N + 63) / 64, heads, B), dim3(256), 0, MVS_STREAM(stream), qkv, out, lse, N, heads, scale2);
    if (cls_row)
        hipLaunchKernelGGL(flash_train_cls_kernel, dim3(heads, B), dim3(256), 0, MVS_STREAM(stream), qkv, (const float*)lse, cls_row,
                           (const float*)nullptr, (float*)nullptr, N, heads, scale2);
    return mvs::finish_launch("mvs_attention_train_fwd_flash");
}

extern "C" int64_t mvs_attention_train_flash_workspace_bytes(int B, int N, int heads) {
    if (B < 1 || N < 1 || heads < 1) return -1;
    return (int64_t)B * heads * N * (int64_t)sizeof(float);
}

extern "C" int mvs_attention_train_bwd_flash(const float* qkv, const float* out, const float* lse, const float* dout, const float* dA_cls, float* dqkv,
                                             void* workspace, int B, int N, int heads, int head_dim, float scale, mvs_stream_t stream) {
    MVS_REQUIRE(qkv && out && lse && dout && dqkv && workspace && B >= 1 && B <= 65535 && N >= 1 && heads >= 1 && heads <= 65535,
                "mvs_attention_train_bwd_flash: bad shape");
    MVS_REQUIRE(head_dim == 64, "mvs_attention_train_bwd_flash: head dimension 64 only (got %d)", head_dim);
    MVS_REQUIRE(aligned16(qkv) && aligned16(out) && aligned16(dout) && aligned16(dqkv) && (reinterpret_cast<uintptr_t>(workspace) & 3) == 0,
                "mvs_attention_train_bwd_flash: qkv, out, dout and dqkv must be 16-byte aligned");
    MVS_REQUIRE((int64_t)N + 63 < ((int64_t)1 << 31), "mvs_attention_train_bwd_flash: N too large");
    const float scale2 = scale * FT_LOG2E;
    float* delta = reinterpret_cast<float*>(workspace);
    hipStream_t s = MVS_STREAM(stream);
    hipLaunchKernelGGL(flash_train_delta_kernel, dim3((N + 15) / 16, heads, B), dim3(256), 0, s, out, dout, delta, N, heads);
    if (dA_cls)
        hipLaunchKernelGGL(flash_train_cls_kernel, dim3(heads, B), dim3(256), 0, s, qkv, lse, (float*)nullptr, dA_cls, delta, N, heads, scale2);
    hipLaunchKernelGGL(flash_train_dkv_kernel, dim3((N + 63) / 64, heads, B), dim3(256), 0, s, qkv, dout, lse, (const float*)delta, dA_cls, dqkv, N, heads,
                       scale, scale2);
    hipLaunchKernelGGL(flash_train_dq_kernel, dim3((N + 63) / 64, heads, B), dim3(256), 0, s, qkv, dout, lse, (const float*)delta, dA_cls, dqkv, N, heads,
                       scale, scale2);
    return mvs::finish_launch("mvs_attention_train_bwd_flash");
}
