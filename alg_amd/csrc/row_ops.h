// Lane primitives of the memory-bound row kernels (norm.hip, wan.hip, hunyuan.hip, llama.hip, wan_vae.hip, vae.hip,
// step_cache.hip, t5.hip; through qk_norm_rope.h the GEMM store loop) and the e4m3 row quantiser (gemm_p6_fp8.hip,
// attention128_fp8.hip and every kernel that quantises a row it has just produced), each defined ONCE; behind it the OCP MXFP4
// block quantiser (gemm_fp4.hip: the row quantiser and the MXFP4 epilogue; norm.hip).  A lane holds eight consecutive elements
// of its row: one 16-byte bf16 access, two for fp32, 8 bytes of e4m3, 4 of e2m1.
#pragma once
#include "common.h"

namespace alg {

// ---- eight elements of a lane ----
__device__ __forceinline__ void unpack8(const uint4 v, float (&f)[8]) {
  const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = __uint_as_float(u[k] << 16);
    f[2 * k + 1] = __uint_as_float(u[k] & 0xffff0000u);
  }
}

__device__ __forceinline__ uint4 pack8(const float (&f)[8]) {
  uint4 v;
  v.x = pack_bf2(f[0], f[1]); v.y = pack_bf2(f[2], f[3]); v.z = pack_bf2(f[4], f[5]); v.w = pack_bf2(f[6], f[7]);
  return v;
}

// eight fp32 values: two 16-byte loads
__device__ __forceinline__ void load8(const float* p, float (&f)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

// ---- reductions over lanes.  The xor butterfly runs from the widest step to 1: for a sum that order is part of the bit
// identity between the one-row and the many-row kernels (and between a kernel and its e4m3 twin) ----
template <int LANES>   // aligned groups of LANES lanes: 64 = the wave, 16 = one 128-wide head vector
__device__ __forceinline__ float xor_sum(float v) {
#pragma unroll
  for (int m = LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
template <int LANES>
__device__ __forceinline__ float xor_max(float v) {
#pragma unroll
  for (int m = LANES / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) { return xor_sum<64>(v); }

// max over the wave of a value >= 0, the same in every lane.  A maximum does not depend on the order it is taken in, so unlike the
// sums of the statistics (whose butterfly order is part of the bit-identity with ln_mod_kernel) it may take the short way: four
// DPP steps inside each row of 16 lanes, two row broadcasts, one v_readlane -- no trip through the LDS crossbar.
// (xor_max<64> is the same value; which kernel takes which is left as it was measured.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_max(float v) {
  const int i = __builtin_bit_cast(int, v);
  return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, CTRL, ROW_MASK, 0xf, false)));
}
__device__ __forceinline__ float wave_max(float v) {
  v = dpp_max<0xB1, 0xf>(v);    // quad_perm [1, 0, 3, 2]
  v = dpp_max<0x4E, 0xf>(v);    // quad_perm [2, 3, 0, 1]
  v = dpp_max<0x141, 0xf>(v);   // row_half_mirror
  v = dpp_max<0x140, 0xf>(v);   // row_mirror: every lane holds its row's maximum
  v = dpp_max<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
  v = dpp_max<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3: lane 63 holds the wave's
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63));
}

// ---- the e4m3 (OCP, max 448) row quantiser: what alg_quantize_fp8_rows writes for a bf16 row, and therefore what every kernel
// that quantises a row still in its registers writes.  scale = amax / 448 (1 for an all-zero row), values times the reciprocal,
// clamped (v_cvt_pk_fp8_f32 saturates nothing), converted two at a time ----
__device__ __forceinline__ float e4m3_scale(float amax) { return amax > 0.0f ? amax * (1.0f / 448.0f) : 1.0f; }

__device__ __forceinline__ float amax8(const float (&f)[8], float amax) {
#pragma unroll
  for (int k = 0; k < 8; ++k) amax = fmaxf(amax, fabsf(f[k]));
  return amax;
}
// (the packed-bf16 forms unpack word by word as they go: the quantiser kernels keep their instruction order)
__device__ __forceinline__ float amax8(const uint4& v, float amax) {
  const uint32_t u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    amax = fmaxf(amax, fabsf(__uint_as_float(u[k] << 16)));
    amax = fmaxf(amax, fabsf(__uint_as_float(u[k] & 0xffff0000u)));
  }
  return amax;
}

__device__ __forceinline__ float e4m3_clamp(float x) { return fminf(fmaxf(x, -448.0f), 448.0f); }
__device__ __forceinline__ uint2 e4m3_cvt8(const float (&f)[8]) {   // f already scaled and clamped
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], hi, true);
  return make_uint2((unsigned)lo, (unsigned)hi);
}
__device__ __forceinline__ uint2 e4m3x8(const float (&v)[8], float inv) {
  float f[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) f[k] = e4m3_clamp(v[k] * inv);
  return e4m3_cvt8(f);
}
__device__ __forceinline__ uint2 e4m3x8(const uint4& v, float inv) {   // eight packed bf16
  const uint32_t u[4] = {v.x, v.y, v.z, v.w};
  float f[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    f[2 * k] = e4m3_clamp(__uint_as_float(u[k] << 16) * inv);
    f[2 * k + 1] = e4m3_clamp(__uint_as_float(u[k] & 0xffff0000u) * inv);
  }
  return e4m3_cvt8(f);
}

// A whole row held by one wave, D = ITERS * 512: v is the row as its bf16 tensor would hold it, amax its reduced maximum
template <int ITERS>
__device__ __forceinline__ void e4m3_row_store(const float (&v)[ITERS][8], float amax, int lane, uint8_t* __restrict__ qr,
                                               float* __restrict__ scale_out) {
  const float qs = e4m3_scale(amax);
  const float inv = 1.0f / qs;
  if (lane == 0) *scale_out = qs;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) *(uint2*)(qr + i * 512 + lane * 8) = e4m3x8(v[i], inv);
}

// ---- the OCP MXFP4 block quantiser (e2m1 elements, one E8M0 scale byte per 32 consecutive elements): what alg_quantize_mxfp4_rows
// writes for a bf16 row, and therefore what every kernel that quantises values still in its registers writes (norm.hip's
// ln_mod_mxfp4_kernel, gemm_fp4.hip's MXFP4 epilogue).  The callers differ only in which lanes share a block, i.e. in how the
// block's amax is gathered; the scale byte, the compare chain and the nibble order are here ----
// E8M0 byte: floor(log2(amax)) - 2 clamped to [-127, 127], + 127.  floor(log2) of a normal number is its exponent field - 127;
// a subnormal amax (field 0) lies below 2^-126 and clamps to byte 0 like field 1 and 2 do.  A zero block writes 127.
__device__ __forceinline__ int mxfp4_scale_byte(float amax) {
  const int ef = (int)(__float_as_uint(amax) >> 23);
  return amax > 0.0f ? (ef > 2 ? ef - 2 : 0) : 127;
}
__device__ __forceinline__ float mxfp4_inv(int e) {   // 2^(127 - e): e <= 252, so a normal number
  return __uint_as_float((uint32_t)(254 - e) << 23);
}
// one element: the sign bit of f (kept on zeros) over the nearest of {0, .5, 1, 1.5, 2, 3, 4, 6}, ties to the even code,
// saturating: one compare per boundary
__device__ __forceinline__ uint32_t e2m1_code(float f, float inv) {
  const float a = fabsf(f) * inv;   // exact (a power of two), or underflows far below the first tie point
  const uint32_t code = (uint32_t)(a > 0.25f) + (uint32_t)(a >= 0.75f) + (uint32_t)(a > 1.25f) + (uint32_t)(a >= 1.75f) +
                        (uint32_t)(a > 2.5f) + (uint32_t)(a >= 3.5f) + (uint32_t)(a > 5.0f);
  return code | ((__float_as_uint(f) >> 28) & 8u);
}
// N consecutive elements (values a bf16 tensor would hold) of a block whose scale byte is e: element k in nibble k
template <int N>
__device__ __forceinline__ uint32_t e2m1_pack(const float (&f)[N], int e) {
  static_assert(N <= 8, "one 32-bit word holds eight e2m1 values");
  const float inv = mxfp4_inv(e);
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) out |= e2m1_code(f[k], inv) << (4 * k);
  return out;
}

// A lane's eight consecutive elements where lane * 8 is the column (the row kernels' mapping): four lanes share an MX block.
// q4 points at the lane's four bytes, scale at the block's byte.
__device__ __forceinline__ void mxfp4_quantize8(const float (&f)[8], uint8_t* __restrict__ q4, uint8_t* __restrict__ scale, int lane) {
  const int e = mxfp4_scale_byte(xor_max<4>(amax8(f, 0.0f)));
  *(uint32_t*)q4 = e2m1_pack(f, e);
  if ((lane & 3) == 0) *scale = (uint8_t)e;
}
__device__ __forceinline__ void mxfp4_quantize8(const uint4 v, uint8_t* __restrict__ q4, uint8_t* __restrict__ scale, int lane) {   // packed bf16
  float f[8];
  unpack8(v, f);
  mxfp4_quantize8(f, q4, scale, lane);
}

// grid of a grid-stride elementwise kernel of 256 threads
inline unsigned grid_for(int64_t total) {
  const int64_t want = (total + 255) / 256;
  return (unsigned)(want < 1 ? 1 : (want > 8192 ? 8192 : want));
}

}  // namespace alg
