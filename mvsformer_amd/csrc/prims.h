// Device primitives every kernel family shares: vector types, wave-uniform buffer descriptors and their loads, the DPP add, and the few
// scalar formulas (activations, bicubic weights, BatchNorm element count) that more than one .hip file evaluates.  A .hip file pulls what
// it needs in with `using mvsprim::name;`.  geometry.h (mvs::), conv_common.h (mvsconv::) and split3.h (mvsx3::) include this file and
// re-export the names their users spell through them; the definitions are here and nowhere else.  Nothing here has state, nothing here is
// host code.
#pragma once
#include <hip/hip_runtime.h>

namespace mvsprim {

using f32x2 = __attribute__((ext_vector_type(2))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// ---- buffer descriptors ------------------------------------------------------------------------------------------------------------
// A wave-uniform descriptor of `bytes` bytes at `base`: the per-lane offset goes in the 32-bit voffset, a wave-uniform one in the scalar
// soffset, so a load costs no 64-bit address arithmetic.  A load beyond `bytes` - or with OOB as its offset, which lies beyond every range
// used in this library (< 2 GiB each) - returns 0 without touching memory: zero padding, tile halos and channel padding without branches.
using rsrc_t = __amdgpu_buffer_rsrc_t;
constexpr unsigned OOB = 0x80000000u;

__device__ __forceinline__ rsrc_t make_rsrc(const float* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, bytes, 0x00020000);
}
// the bf16 / packed-operand form (bf16_train.hip): any element type
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}

__device__ __forceinline__ float buf_load(rsrc_t r, unsigned voff_bytes, unsigned soff_bytes) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff_bytes, soff_bytes, 0));
}
__device__ __forceinline__ f32x4 buf_load4(rsrc_t r, unsigned voff_bytes) {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff_bytes, 0, 0));
}
// buf_load with the cache policy AUX (aux of raw_buffer_load: 0 = default, 2 = nt): the staging / skip-tensor loads of the split-form 3-D kernels
template <int AUX>
__device__ __forceinline__ float stage_load(rsrc_t r, unsigned voff_bytes, unsigned soff_bytes) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff_bytes, soff_bytes, AUX));
}

// ---- cross-lane ----------------------------------------------------------------------------------------------------------------------
// v + (v of the lane the DPP control CTRL selects): a full-rate VALU operation, no LDS crossbar traffic (the ds_bpermute form of
// __shfl_xor).  0xB1 / 0x4E = quad_perm xor 1 / xor 2, 0x141 = row_half_mirror (i <-> 7-i), 0x140 = row_mirror (i <-> 15-i).
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v) {
    const int o = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true);
    return v + __builtin_bit_cast(float, o);
}

// ---- scalar formulas -----------------------------------------------------------------------------------------------------------------
// x * sigmoid(x) with the hardware exp2 / reciprocal (a few ulp; the epilogue shares the fp32 pipe with the MFMAs, an IEEE divide costs 10 slots)
__device__ __forceinline__ float swish(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }   // v_pk_fma_f32

// ATen's cubic convolution weights with A = -0.75 (upsample_bicubic2d): |x| <= 1 and 1 < |x| < 2
__device__ __forceinline__ float cc1(float x) { return ((-0.75f + 2.0f) * x - (-0.75f + 3.0f)) * x * x + 1.0f; }
__device__ __forceinline__ float cc2(float x) { return ((-0.75f * x - 5.0f * -0.75f) * x + 8.0f * -0.75f) * x - 4.0f * -0.75f; }

// Element count per channel of a BatchNorm: a host value, or (SyncBatchNorm) two floats {n / 4096, n % 4096} that rode through the same
// all-reduce as the sums - each stays exactly representable in fp32 up to 2^36 elements, so the total is exact and the
// host never has to read it back.
__device__ __forceinline__ double resolve_count(double count_host, const float* __restrict__ count_dev) {
    return count_dev ? (double)count_dev[0] * 4096.0 + (double)count_dev[1] : count_host;
}

}  // namespace mvsprim
