// HBM-bound kernels specific to the HunyuanVideo DiT forward (diffusers
// HunyuanVideoTransformer3DModel, call site pipeline_hunyuan_video_image2video_lowpass.py:1243-1252): per-head RMSNorm of
// q / k fused with the 3-axis rotary embedding of the latent tokens, the masked mean that pools the prompt for the token
// refiner, SiLU of the conditioning vectors.  Everything else of that forward reuses the CogVideoX / Wan kernels.
#include "common.h"
#include "rownorm_host.h"
#include "row_ops.h"

namespace alg {
namespace hy {

// One 128-wide head vector, 16 lanes with 8 elements each (`sub` = the lane's place among them):
// o = rope( bf16( bf16(x * rsqrt(mean_head(x^2) + eps)) * w ) ) in fp32, before its last rounding.  rope = x * cos + rot(x) * sin
// over interleaved pairs, fp32 tables [.][128] -- only on tokens < rope_tokens.  Written once for the kernel and its e4m3 twin.
__device__ __forceinline__ void headnorm_rope_vec(const bf16_t* p, const bf16_t* w, const float* cos_tab, const float* sin_tab,
                                                  int tok, int sub, int rope_tokens, float eps, float (&o)[8]) {
  float v[8], wv[8];
  unpack8(*(const uint4*)p, v);
  unpack8(*(const uint4*)(w + sub * 8), wv);
  float q = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) q = fmaf(v[k], v[k], q);
  q = xor_sum<16>(q);
  const float rstd = rsqrtf(q * (1.0f / 128.0f) + eps);
#pragma unroll
  for (int k = 0; k < 8; ++k) o[k] = rbf(rbf(v[k] * rstd) * wv[k]);
  if (cos_tab && tok < rope_tokens) {
    float cv[8], sv[8];
    load8(cos_tab + (int64_t)tok * 128 + sub * 8, cv);
    load8(sin_tab + (int64_t)tok * 128 + sub * 8, sv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = o[2 * j], b = o[2 * j + 1];
      o[2 * j] = a * cv[2 * j] + (-b) * sv[2 * j];
      o[2 * j + 1] = b * cv[2 * j + 1] + a * sv[2 * j + 1];
    }
  }
}

// in place on rows of `heads` 128-wide head vectors; rope only on tokens < rope_tokens of each batch.
__global__ __launch_bounds__(256) void headnorm_rope_kernel(bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                            const float* __restrict__ cos_tab,
                                                            const float* __restrict__ sin_tab, int64_t x_rs,
                                                            int64_t x_bs, int64_t total_rows, int rows, int heads,
                                                            int rope_tokens, float eps) {
  const int64_t vec = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;  // (row, head) index
  const int sub = threadIdx.x & 15;
  if (vec >= total_rows * heads) return;
  const int64_t row = vec / heads;
  const int head = (int)(vec - row * heads);
  const int tok = (int)(row % rows);
  bf16_t* p = x + (row / rows) * x_bs + (int64_t)tok * x_rs + head * 128 + sub * 8;
  float o[8];
  headnorm_rope_vec(p, w, cos_tab, sin_tab, tok, sub, rope_tokens, eps, o);
  *(uint4*)p = pack8(o);
}

// headnorm_rope_kernel writing OCP e4m3 for alg_flash_attn_d128_fp8 instead of updating x (x is only read): the bf16-rounded head
// vector is quantised in registers exactly as a quantiser pass over the bf16 tensor would (row_ops.h).  head_scale == nullptr:
// scale[b * scale_bs + tok * heads + head] = amax / 448 of the head vector (the Q operand); otherwise the given scale of
// head_scale[b * heads + head] is used (the K operand) and `scale` is not written.
__global__ __launch_bounds__(256) void headnorm_rope_fp8_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ w,
                                                                const float* __restrict__ cos_tab,
                                                                const float* __restrict__ sin_tab, int64_t x_rs, int64_t x_bs,
                                                                int64_t total_rows, int rows, int heads, int rope_tokens, float eps,
                                                                uint8_t* __restrict__ q8, int64_t q8_rs, int64_t q8_bs,
                                                                float* __restrict__ scale, int64_t scale_bs,
                                                                const float* __restrict__ head_scale) {
  const int64_t vec = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;  // (row, head) index
  const int sub = threadIdx.x & 15;
  if (vec >= total_rows * heads) return;
  const int64_t row = vec / heads;
  const int head = (int)(vec - row * heads);
  const int tok = (int)(row % rows);
  const int64_t bidx = row / rows;
  const bf16_t* p = x + bidx * x_bs + (int64_t)tok * x_rs + head * 128 + sub * 8;
  float o[8];
  headnorm_rope_vec(p, w, cos_tab, sin_tab, tok, sub, rope_tokens, eps, o);
  float amax = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    o[k] = rbf(o[k]);   // what alg_headnorm_rope stores
    amax = fmaxf(amax, fabsf(o[k]));
  }
  float sc;
  if (head_scale) {
    sc = head_scale[bidx * heads + head];
  } else {
    // (open-coded, not xor_max<16>: through the template hipcc words one scalar branch of this kernel the other way round, and
    // this kernel's device code is held byte for byte)
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
    sc = e4m3_scale(amax);
    if (sub == 0) scale[bidx * scale_bs + (int64_t)tok * heads + head] = sc;
  }
  *(uint2*)(q8 + bidx * q8_bs + (int64_t)tok * q8_rs + head * 128 + sub * 8) = e4m3x8(o, 1.0f / sc);
}

// out[b][d] = bf16( sum_{l < valid[b]} x[b][l][d] / valid[b] )   (HunyuanVideoTokenRefiner pooled prompt)
__global__ __launch_bounds__(256) void masked_mean_kernel(const bf16_t* __restrict__ x, const int* __restrict__ valid,
                                                          bf16_t* __restrict__ out, int B, int L, int D) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (int64_t)B * D) return;
  const int b = (int)(e / D), d = (int)(e % D);
  const int n = valid[b];
  float acc = 0.0f;
  for (int l = 0; l < n; ++l) acc += bf2f(x[((int64_t)b * L + l) * D + d]);
  out[e] = f2bf(acc / (float)n);
}

__global__ __launch_bounds__(256) void silu_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, int64_t numel) {
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < numel; e += (int64_t)gridDim.x * blockDim.x) {
    const float v = bf2f(x[e]);
    y[e] = f2bf(v / (1.0f + __expf(-v)));
  }
}

}  // namespace hy
}  // namespace alg

using namespace alg;

extern "C" int alg_headnorm_rope(void* x, const void* weight, const float* cos_tab, const float* sin_tab,
                                 int64_t x_rstride, int64_t x_bstride, int batch, int rows, int heads, int rope_tokens,
                                 float eps, void* stream) {
  NormRopeArgs a = {};
  a.per_head = true; a.x = x; a.weight = weight; a.cos_tab = cos_tab; a.sin_tab = sin_tab;
  a.x_rstride = x_rstride; a.x_bstride = x_bstride; a.batch = batch; a.rows = rows; a.width = heads;
  if (const int rc = norm_rope_check(a, "alg_headnorm_rope")) return rc == ROW_EMPTY ? ALG_OK : rc;
  hipLaunchKernelGGL(hy::headnorm_rope_kernel, dim3((unsigned)norm_rope_blocks(a)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)x,
                     (const bf16_t*)weight, cos_tab, sin_tab, x_rstride, x_bstride, norm_rope_total(a), rows, heads,
                     rope_tokens, eps);
  return check_launch("alg_headnorm_rope");
}

extern "C" int alg_headnorm_rope_fp8(const void* x, const void* weight, const float* cos_tab, const float* sin_tab,
                                     int64_t x_rstride, int64_t x_bstride, int batch, int rows, int heads, int rope_tokens,
                                     float eps, void* q8, int64_t q8_rstride, int64_t q8_bstride, float* scale,
                                     int64_t scale_bstride, const float* head_scale, void* stream) {
  NormRopeArgs a = {};
  a.per_head = true; a.x = x; a.weight = weight; a.cos_tab = cos_tab; a.sin_tab = sin_tab;
  a.x_rstride = x_rstride; a.x_bstride = x_bstride; a.batch = batch; a.rows = rows; a.width = heads;
  a.fp8 = true; a.q8 = q8; a.q8_rstride = q8_rstride; a.q8_bstride = q8_bstride; a.scale = scale; a.head_scale = head_scale;
  if (const int rc = norm_rope_check(a, "alg_headnorm_rope_fp8")) return rc == ROW_EMPTY ? ALG_OK : rc;
  hipLaunchKernelGGL(hy::headnorm_rope_fp8_kernel, dim3((unsigned)norm_rope_blocks(a)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (const bf16_t*)weight, cos_tab, sin_tab, x_rstride, x_bstride, norm_rope_total(a), rows,
                     heads, rope_tokens, eps, (uint8_t*)q8, q8_rstride, q8_bstride, scale, scale_bstride, head_scale);
  return check_launch("alg_headnorm_rope_fp8");
}

extern "C" int alg_masked_mean(const void* x, const int* valid, void* out, int batch, int L, int D, void* stream) {
  if (!x || !valid || !out || batch <= 0 || L <= 0 || D <= 0) {
    set_error("alg_masked_mean: bad argument");
    return ALG_EINVAL;
  }
  const int64_t total = (int64_t)batch * D;
  hipLaunchKernelGGL(hy::masked_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, valid, (bf16_t*)out, batch, L, D);
  return check_launch("alg_masked_mean");
}

extern "C" int alg_silu(const void* x, void* y, int64_t numel, void* stream) {
  if (numel < 0) {
    set_error("alg_silu: bad argument");
    return ALG_EINVAL;
  }
  if (numel == 0) return ALG_OK;
  if (!x || !y) {
    set_error("alg_silu: null pointer");
    return ALG_EINVAL;
  }
  int64_t want = (numel + 255) / 256;
  hipLaunchKernelGGL(hy::silu_kernel, dim3((unsigned)(want > 4096 ? 4096 : want)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, (bf16_t*)y, numel);
  return check_launch("alg_silu");
}
