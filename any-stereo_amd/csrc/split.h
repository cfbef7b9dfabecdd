// The split-precision arithmetic of every GEMM-shaped kernel (DESIGN.md "split"), written once.  Device code; include
// after common.h.  An fp32 operand is carried as two fp16 values, x = hi + lo/2048 with hi = fp16(x) and
// lo = fp16((x - hi) * 2048); a product is three v_mfma_f32_32x32x16_f16 (hi.hi into acc_h; hi.lo and lo.hi into acc_x)
// and the result is acc_h + acc_x/2048.  Kernels meet bit for bit because they all compile THESE expressions: a new
// kernel includes this header, it does not re-type them.
#pragma once
#include "common.h"

namespace as {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x2 = __attribute__((ext_vector_type(2))) float;
using half8 = __attribute__((ext_vector_type(8))) _Float16;
using half4v = __attribute__((ext_vector_type(4))) _Float16;
using half2v = __attribute__((ext_vector_type(2))) _Float16;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;  // wgrad.hip's bf16 MFMA operand

constexpr float kSplitScale = 2048.f, kSplitInv = 1.f / kSplitScale, kF16Max = 65504.f;

// ---- the operand split, two flavours that differ in how |x| >= 65504 saturates ---------------------------------------
// mode:  split_hi / split_lo of x itself.  The KERNEL must have called fp16_saturate_mode() (common.h); then an
//        out-of-range x converts to +-65504 and a NaN stays a NaN.  Without the mode bit hi = inf, lo = NaN.
// clamp: split_hi / split_lo of clamp_f16(x), a v_med3_f32 to +-65504; needs no mode bit, and a NaN becomes finite.
// split_mode8 and split_part_mode / split_part_clamp carry the flavour in their names; a scalar site shows it by calling
// clamp_f16 or not.
// Either way the caller keeps a running max |x| and reports it once with note_split_overflow (common.h).
// (liif_fused.hip's split8 / split8_pos are a third, packed round-toward-zero split, ~2^-20 per operand: not these.)
__device__ __forceinline__ float clamp_f16(float x) { return __builtin_amdgcn_fmed3f(x, -kF16Max, kF16Max); }
__device__ __forceinline__ _Float16 split_hi(float x) { return (_Float16)x; }
__device__ __forceinline__ _Float16 split_lo(float x, _Float16 hi) { return (_Float16)((x - (float)hi) * kSplitScale); }

// 8 values -> a half8 pair (mode flavour), and the thread's running max |x| that goes with them, pairwise: one v_max3
// per two values.  Two calls, in the order the kernel had them: the compiler's schedule follows it.  amax goes in and
// comes out by value, and a site that builds `v` in the same function and was tuned with its own loop (conv_split_kernel,
// lookup.hip) keeps that loop over split_hi / split_lo / amax2: a local handed to a function by reference, even an
// inlined one, is promoted to registers later, and the schedule of a tuned kernel comes out different.
__device__ __forceinline__ float amax2(float amax, float a, float b) { return fmaxf(amax, fmaxf(fabsf(a), fabsf(b))); }
__device__ __forceinline__ float amax8(const float (&v)[8], float amax) {
#pragma unroll
  for (int j = 0; j < 8; j += 2) amax = amax2(amax, v[j], v[j + 1]);
  return amax;
}
__device__ __forceinline__ void split_mode8(const float (&v)[8], half8& hi, half8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const _Float16 hj = split_hi(v[j]);
    hi[j] = hj;
    lo[j] = split_lo(v[j], hj);
  }
}

// component hl (0 = hi, 1 = lo) of x: the tail of the weight-image pack kernels
__device__ __forceinline__ _Float16 split_part_mode(float x, int hl) {
  const _Float16 hi = split_hi(x);
  return hl == 0 ? hi : split_lo(x, hi);
}
__device__ __forceinline__ _Float16 split_part_clamp(float x, int hl) { return split_part_mode(clamp_f16(x), hl); }

// ---- the join, two forms that round differently ----------------------------------------------------------------------
__device__ __forceinline__ float join(float h, float x) { return h + x * kSplitInv; }
__device__ __forceinline__ float join_fma(float h, float x) { return fmaf(x, kSplitInv, h); }

// ---- one product: hi.hi -> acc_h; hi.lo and lo.hi -> acc_x.  Accumulators go in and come out by value (through
// references the compiler schedules some callers differently).  Only where the three MFMAs stand together; the
// hand-interleaved schedules (AS_SPLIT_STEP_IL, AS_MM_HH/HX/LH, PW_CHUNK, the fast16 paths) place the builtins themselves.
__device__ __forceinline__ f32x16 split_mfma_h(f32x16 acc_h, half8 a_hi, half8 b_hi) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_hi, acc_h, 0, 0, 0);
}
__device__ __forceinline__ f32x16 split_mfma_x(f32x16 acc_x, half8 a_hi, half8 a_lo, half8 b_hi, half8 b_lo) {
  acc_x = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi, b_lo, acc_x, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo, b_hi, acc_x, 0, 0, 0);
}

// ---- activation codes of the C ABI (AS_ACT_*).  AS_ACT_GELU is honoured only with GELU = true (backbone.hip); the
// convolutions pass it through unchanged, as they always have.
template <bool GELU = false>
__device__ __forceinline__ float act_apply(float v, int act) {
  switch (act) {
    case AS_ACT_RELU: return fmaxf(v, 0.f);
    case AS_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
    case AS_ACT_TANH: return tanhf(v);
    case AS_ACT_RELU6: return fminf(fmaxf(v, 0.f), 6.f);
    case AS_ACT_LEAKY: return v >= 0.f ? v : 0.01f * v;
    case AS_ACT_GELU: return GELU ? 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)) : v;
    default: return v;
  }
}

// ---- 32-bit raw-buffer access: an offset past the descriptor's range loads 0 / drops the store.  The out-of-range
// sentinel offsets stay with each kernel (they depend on its offset arithmetic).
__device__ __forceinline__ float bload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff = 0) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}
__device__ __forceinline__ void bstore(__amdgpu_buffer_rsrc_t r, unsigned voff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, (int)voff, 0, 0);
}

}  // namespace as
