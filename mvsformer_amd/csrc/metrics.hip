// Depth metrics of a batch - the reference's utils.py:148-182 (Thres_metrics, AbsDepthError_metrics under compute_metrics_for_each_image) and
// the DictAverageMeter update of utils.py:119-145 - in one pass over depth_est, depth_gt and the mask.
//
// The reference gathers the valid pixels of each image twice per metric (boolean-mask indexing), subtracts, compares, takes a mean and ends
// every metric in an .item().  Here one lane owns four consecutive pixels: the error |est - gt| is formed in fp32 as the reference forms it,
// valid pixels and pixels above each threshold are counted per wavefront with __ballot + popcount (exact integers), the errors are added in
// double (a lane's four, then a shuffle tree in a fixed order).  One row per block, then mvs_depth_metrics' two finalize launches add the
// rows of an image in a fixed order (one block per image) and the images of the batch (one block); the last one also advances a meter.
// No float atomics anywhere: two runs give the same bits.
//
// Loads: an image's maps start at est + b * HW, which is 16-byte aligned only by luck (HW odd, or a view at a storage offset).  The block's
// pixel index is therefore shifted by `phase` = the image's distance (in floats) from the 16-byte boundary below it, so that every lane's
// quad starts ON a boundary; where depth_gt and the mask share that phase the quad is three vector loads (two and a dword for a byte mask),
// everywhere else - the head and the tail of the image, or maps of different phases - four bounds-checked scalar loads per map.
#include "block_ops.h"

namespace {

constexpr int MET_THREADS = 256, MET_PPT = 4, MET_P = MET_THREADS * MET_PPT, MET_MAXK = MVS_DEPTH_METRICS_MAX_K;
static_assert(MET_P == MVS_DEPTH_METRICS_BLOCK_PIXELS, "the public header names the block's pixels");

struct MetRow {                       // one block's partial sums: 48 bytes = 12 floats of acc
    double sum;                       // sum of e over the valid pixels inside the band
    uint32_t n_valid, n_band;
    uint32_t above[MET_MAXK];
};
static_assert(sizeof(MetRow) == 48, "MetRow layout");
constexpr int MET_ROW_FLOATS = sizeof(MetRow) / sizeof(float);
constexpr int MET_NCNT = 2 + MET_MAXK;

__device__ __forceinline__ unsigned phase_of(const void* p) { return (unsigned)(((uintptr_t)p >> 2) & 3); }

template <bool MASK8>
__global__ __launch_bounds__(MET_THREADS) void depth_metrics_kernel(const float* __restrict__ est, const float* __restrict__ gt,
                                                                    const void* __restrict__ mask, const float* __restrict__ thr, int K,
                                                                    long long HW, int use_band, float lo, float hi, MetRow* __restrict__ rows) {
    __shared__ double sred[MET_THREADS / 64];
    __shared__ uint32_t cred[MET_NCNT][MET_THREADS / 64];
    const int b = blockIdx.y;
    const float* e_img = est + (size_t)b * HW;
    const float* g_img = gt + (size_t)b * HW;
    const float* mf_img = reinterpret_cast<const float*>(mask) + (size_t)b * HW;
    const uint8_t* m8_img = reinterpret_cast<const uint8_t*>(mask) + (size_t)b * HW;
    const unsigned phase = phase_of(e_img);
    const bool vec_ok = phase_of(g_img) == phase && (MASK8 ? (((uintptr_t)m8_img - phase) & 3) == 0 : phase_of(mf_img) == phase);
    const long long p0 = (long long)blockIdx.x * MET_P + (long long)threadIdx.x * MET_PPT - (long long)phase;     // first pixel of the quad
    float ev[MET_PPT], gv[MET_PPT];
    bool val[MET_PPT];
    if (vec_ok && p0 >= 0 && p0 + MET_PPT <= HW) {                // a whole quad on a 16-byte boundary of all three maps
        const float4 e4 = *reinterpret_cast<const float4*>(e_img + p0);
        const float4 g4 = *reinterpret_cast<const float4*>(g_img + p0);
        ev[0] = e4.x, ev[1] = e4.y, ev[2] = e4.z, ev[3] = e4.w;
        gv[0] = g4.x, gv[1] = g4.y, gv[2] = g4.z, gv[3] = g4.w;
        if (MASK8) {
            const uint32_t m4 = *reinterpret_cast<const uint32_t*>(m8_img + p0);
#pragma unroll
            for (int j = 0; j < MET_PPT; ++j) val[j] = ((m4 >> (8 * j)) & 0xffu) != 0;
        } else {
            const float4 m4 = *reinterpret_cast<const float4*>(mf_img + p0);
            val[0] = m4.x > 0.5f, val[1] = m4.y > 0.5f, val[2] = m4.z > 0.5f, val[3] = m4.w > 0.5f;
        }
    } else {
#pragma unroll
        for (int j = 0; j < MET_PPT; ++j) {
            const long long p = p0 + j;
            const bool in = p >= 0 && p < HW;
            ev[j] = in ? e_img[p] : 0.0f;
            gv[j] = in ? g_img[p] : 0.0f;
            val[j] = in && (MASK8 ? m8_img[p] != 0 : mf_img[p] > 0.5f);
        }
    }
    float err[MET_PPT];
    bool band[MET_PPT];
    double s = 0.0;
    uint32_t cnt[MET_NCNT];
#pragma unroll
    for (int c = 0; c < MET_NCNT; ++c) cnt[c] = 0;
#pragma unroll
    for (int j = 0; j < MET_PPT; ++j) {
        err[j] = fabsf(ev[j] - gv[j]);                            // fp32, as the reference; used only where val[j] (a select, never a product)
        band[j] = val[j] && (!use_band || (err[j] >= lo && err[j] <= hi));
        s += band[j] ? (double)err[j] : 0.0;
        cnt[0] += blk::ballot_count(val[j]);
        cnt[1] += blk::ballot_count(band[j]);
    }
#pragma unroll
    for (int k = 0; k < MET_MAXK; ++k) {
        if (k < K) {                                              // block-uniform
            const float t = thr[(size_t)b * K + k];
#pragma unroll
            for (int j = 0; j < MET_PPT; ++j) cnt[2 + k] += blk::ballot_count(val[j] && err[j] > t);
        }
    }
    blk::block_sum_put(s, sred);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < MET_NCNT; ++c) cred[c][threadIdx.x >> 6] = cnt[c];         // every lane of the wavefront holds the same counts
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        MetRow r;
        r.sum = blk::sum4(sred);
        r.n_valid = blk::sum4(cred[0]);
        r.n_band = blk::sum4(cred[1]);
#pragma unroll
        for (int k = 0; k < MET_MAXK; ++k) r.above[k] = blk::sum4(cred[2 + k]);
        rows[(size_t)b * gridDim.x + blockIdx.x] = r;
    }
}

// one block per image: its nblk rows in a fixed order -> counts [2+K], per_image [1+K]
__global__ __launch_bounds__(MET_THREADS) void depth_metrics_image_kernel(const MetRow* __restrict__ rows, int nblk, int K, int use_band,
                                                                          int32_t* __restrict__ counts, float* __restrict__ per_image) {
    __shared__ double sred[MET_THREADS / 64];
    __shared__ unsigned long long cred[MET_NCNT][MET_THREADS / 64];
    const int b = blockIdx.x;
    const MetRow* r = rows + (size_t)b * nblk;
    double s = 0.0;
    unsigned long long cnt[MET_NCNT];
#pragma unroll
    for (int c = 0; c < MET_NCNT; ++c) cnt[c] = 0;
    for (int i = threadIdx.x; i < nblk; i += MET_THREADS) {
        s += r[i].sum;
        cnt[0] += r[i].n_valid;
        cnt[1] += r[i].n_band;
#pragma unroll
        for (int k = 0; k < MET_MAXK; ++k) cnt[2 + k] += r[i].above[k];
    }
    blk::block_sum_put(s, sred);
#pragma unroll
    for (int c = 0; c < MET_NCNT; ++c) blk::block_sum_put(cnt[c], cred[c]);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = blk::sum4(sred);
        unsigned long long tot[MET_NCNT];
#pragma unroll
        for (int c = 0; c < MET_NCNT; ++c) tot[c] = blk::sum4(cred[c]);
        const double n = (double)tot[0], nb = (double)tot[1];
        int32_t* co = counts + (size_t)b * (2 + K);
        float* po = per_image + (size_t)b * (1 + K);
        co[0] = (int32_t)tot[0];
        co[1] = (int32_t)tot[1];
        // utils.py:175-182: with a band an empty selection gives 0; without one the mean over nothing is NaN (0 / 0)
        po[0] = use_band ? (tot[1] ? (float)(sum / nb) : 0.0f) : (float)(sum / n);
        for (int k = 0; k < K; ++k) {
            co[2 + k] = (int32_t)tot[2 + k];
            po[1 + k] = (float)((double)tot[2 + k] / n);          // n = 0: NaN, as torch.mean of an empty tensor
        }
    }
}

// the batch: lane j adds per_image[:, j] in image order (torch.stack(results).mean()); then the meter
__global__ __launch_bounds__(64) void depth_metrics_batch_kernel(const float* __restrict__ per_image, int B, int K, float* __restrict__ batch,
                                                                 double* __restrict__ meter_sums, double* __restrict__ meter_count, double meter_n) {
    const int j = threadIdx.x;
    if (j <= K) {
        double a = 0.0;
        for (int b = 0; b < B; ++b) a += (double)per_image[(size_t)b * (1 + K) + j];
        const float m = (float)(a / (double)B);
        batch[j] = m;
        if (meter_sums) meter_sums[j] += (double)m;               // DictAverageMeter adds the fp32 value as a Python float
    }
    if (j == 0 && meter_count) meter_count[0] += meter_n;
}

long long met_blocks(long long HW, long long phase) { return mvs::ceil_div(HW + phase, (long long)MET_P); }

}  // namespace

extern "C" int mvs_depth_metrics_block_pixels(void) { return MET_P; }

extern "C" int64_t mvs_depth_metrics_acc_floats(int B, int64_t HW) {
    // rows for the worst phase (3 floats past a 16-byte boundary)
    return (B < 1 || HW < 1 || HW > INT32_MAX) ? -1 : (int64_t)MET_ROW_FLOATS * B * met_blocks(HW, 3);
}

extern "C" int mvs_depth_metrics(const float* depth_est, const float* depth_gt, const void* mask, int mask_is_byte, const float* thresholds, int B,
                                 int K, int64_t HW, int use_band, float band_lo, float band_hi, float* acc, int32_t* counts, float* per_image,
                                 float* batch, double* meter_sums, double* meter_count, double meter_n, mvs_stream_t stream) {
    MVS_REQUIRE(K >= 0 && K <= MET_MAXK, "mvs_depth_metrics: K=%d thresholds, 0..%d are built", K, MET_MAXK);
    MVS_REQUIRE(B >= 1 && B <= 65535 && HW >= 1 && HW <= INT32_MAX, "mvs_depth_metrics: bad shape B=%d HW=%lld", B, (long long)HW);
    MVS_REQUIRE(depth_est && depth_gt && mask && acc && counts && per_image && batch && (K == 0 || thresholds), "mvs_depth_metrics: null pointer");
    MVS_REQUIRE(((uintptr_t)depth_est & 3) == 0 && ((uintptr_t)depth_gt & 3) == 0 && (mask_is_byte || ((uintptr_t)mask & 3) == 0),
                "mvs_depth_metrics: an fp32 map is not 4-byte aligned");
    MVS_REQUIRE(((uintptr_t)acc & 7) == 0 && ((uintptr_t)meter_sums & 7) == 0 && ((uintptr_t)meter_count & 7) == 0,
                "mvs_depth_metrics: acc and the meter must be 8-byte aligned");
    // the largest phase of an image decides the blocks per image; never more than mvs_depth_metrics_acc_floats sized
    long long phase = 0;
    for (int b = 0; b < B && phase < 3; ++b) {
        const long long ph = (long long)((((uintptr_t)depth_est >> 2) + (unsigned long long)b * (unsigned long long)HW) & 3);
        phase = ph > phase ? ph : phase;
    }
    const int nblk = (int)met_blocks(HW, phase);
    hipStream_t s = MVS_STREAM(stream);
    MetRow* rows = reinterpret_cast<MetRow*>(acc);
    dim3 grid((unsigned)nblk, (unsigned)B);
    if (mask_is_byte)
        hipLaunchKernelGGL(depth_metrics_kernel<true>, grid, dim3(MET_THREADS), 0, s, depth_est, depth_gt, mask, thresholds, K, (long long)HW,
                           use_band, band_lo, band_hi, rows);
    else
        hipLaunchKernelGGL(depth_metrics_kernel<false>, grid, dim3(MET_THREADS), 0, s, depth_est, depth_gt, mask, thresholds, K, (long long)HW,
                           use_band, band_lo, band_hi, rows);
    hipLaunchKernelGGL(depth_metrics_image_kernel, dim3((unsigned)B), dim3(MET_THREADS), 0, s, rows, nblk, K, use_band, counts, per_image);
    hipLaunchKernelGGL(depth_metrics_batch_kernel, dim3(1), dim3(64), 0, s, per_image, B, K, batch, meter_sums, meter_count, meter_n);
    return mvs::finish_launch("mvs_depth_metrics");
}
