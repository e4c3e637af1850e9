// fp8 (OCP e4m3) operands on the ping-pong schedule (see gemm_kernel.h) + the row-wise quantiser that feeds it.
#include "gemm_kernel.h"
#include "row_ops.h"

namespace alg {
int launch_gemm_p6_fp8(const alg_gemm_args* a, int m_tiles, int n_tiles, int64_t nwg, hipStream_t s) {
  return launch_gemm<6, 4, true>(a, m_tiles, n_tiles, nwg, s);
}

// one wave per row: amax over the row, then e4m3 conversion of x / scale -- the quantiser itself is row_ops.h's
__device__ __forceinline__ float row_scale_store(float amax, int lane, float* __restrict__ scale_out) {
  const float sc = e4m3_scale(xor_max<64>(amax));
  if (lane == 0) *scale_out = sc;
  return 1.0f / sc;
}
// the two-pass form, any K % 8 == 0: xr / qr are the row's first element
__device__ __forceinline__ void quantize_row_loop(const bf16_t* __restrict__ xr, uint8_t* __restrict__ qr,
                                                  float* __restrict__ scale_out, int K, int lane) {
  float amax = 0.0f;
  for (int c = lane * 8; c < K; c += 512) amax = amax8(*(const uint4*)(xr + c), amax);
  const float inv = row_scale_store(amax, lane, scale_out);
  for (int c = lane * 8; c < K; c += 512) *(uint2*)(qr + c) = e4m3x8(*(const uint4*)(xr + c), inv);
}
// The same arithmetic with the whole row in registers (round 5): K = ITERS * 512, every 16-byte load of the row in flight at once, ONE
// pass over the row instead of two (the loop form above reads it for the amax and again for the conversion).  Bit-identical.
template <int ITERS>
__device__ __forceinline__ void quantize_row_reg(const bf16_t* __restrict__ xr, uint8_t* __restrict__ qr,
                                                 float* __restrict__ scale_out, int lane) {
  uint4 v[ITERS];
#pragma unroll
  for (int i = 0; i < ITERS; ++i) v[i] = *(const uint4*)(xr + i * 512 + lane * 8);
  float amax = 0.0f;
#pragma unroll
  for (int i = 0; i < ITERS; ++i) amax = amax8(v[i], amax);
  const float inv = row_scale_store(amax, lane, scale_out);
#pragma unroll
  for (int i = 0; i < ITERS; ++i) *(uint2*)(qr + i * 512 + lane * 8) = e4m3x8(v[i], inv);
}

__global__ __launch_bounds__(256) void quantize_fp8_rows_kernel(const bf16_t* __restrict__ x, int64_t x_rs,
                                                                uint8_t* __restrict__ q, float* __restrict__ scale,
                                                                int64_t rows, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  quantize_row_loop(x + row * x_rs, q + row * (int64_t)K, scale + row, K, lane);
}
template <int ITERS>
__global__ __launch_bounds__(256) void quantize_fp8_rows_reg_kernel(const bf16_t* __restrict__ x, int64_t x_rs,
                                                                    uint8_t* __restrict__ q, float* __restrict__ scale,
                                                                    int64_t rows) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  quantize_row_reg<ITERS>(x + row * x_rs, q + row * (int64_t)(ITERS * 512), scale + row, lane);
}

// alg_quantize_fp8_rows_batched: row r of batch item b starts at x + b * x_bs + r * x_rs (rows inside a wider, batch-strided
// buffer); q and scale are contiguous over all batch * rows rows.  One launch for all items, the same two row forms.
__global__ __launch_bounds__(256) void quantize_fp8_rows_batched_kernel(const bf16_t* __restrict__ x, int64_t x_bs, int64_t x_rs,
                                                                        uint8_t* __restrict__ q, float* __restrict__ scale,
                                                                        int64_t total_rows, int rows, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= total_rows) return;
  const int64_t b = row / rows;
  quantize_row_loop(x + b * x_bs + (row - b * rows) * x_rs, q + row * (int64_t)K, scale + row, K, lane);
}
template <int ITERS>
__global__ __launch_bounds__(256) void quantize_fp8_rows_batched_reg_kernel(const bf16_t* __restrict__ x, int64_t x_bs,
                                                                            int64_t x_rs, uint8_t* __restrict__ q,
                                                                            float* __restrict__ scale, int64_t total_rows,
                                                                            int rows) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= total_rows) return;
  const int64_t b = row / rows;
  quantize_row_reg<ITERS>(x + b * x_bs + (row - b * rows) * x_rs, q + row * (int64_t)(ITERS * 512), scale + row, lane);
}
}  // namespace alg

using namespace alg;

extern "C" int alg_quantize_fp8_rows(const void* x, int64_t x_rstride, void* q, float* scale, int64_t rows, int K,
                                     void* stream) {
  if (rows < 0 || K <= 0 || K % 8 || x_rstride % 8) {
    set_error("alg_quantize_fp8_rows: bad shape rows=%lld K=%d (K %% 8 == 0)", (long long)rows, K);
    return ALG_EINVAL;
  }
  if (rows == 0) return ALG_OK;
  if (!x || !q || !scale || ((uintptr_t)x & 15) || ((uintptr_t)q & 7)) {
    set_error("alg_quantize_fp8_rows: null or misaligned pointer");
    return ALG_EINVAL;
  }
  const dim3 grid((unsigned)((rows + 3) / 4)), blk(256);
#define ALG_QROWS(I)                                                                                                              \
  case I:                                                                                                                         \
    hipLaunchKernelGGL(quantize_fp8_rows_reg_kernel<I>, grid, blk, 0, (hipStream_t)stream, (const bf16_t*)x, x_rstride, (uint8_t*)q, \
                       scale, rows);                                                                                              \
    return check_launch("alg_quantize_fp8_rows");
  if (K % 512 == 0) switch (K / 512) {   // the widths of the Wan blocks (5120, 13824) and their neighbours: the row lives in registers
      ALG_QROWS(6) ALG_QROWS(8) ALG_QROWS(10) ALG_QROWS(12) ALG_QROWS(16) ALG_QROWS(24) ALG_QROWS(27)
      default: break;
    }
#undef ALG_QROWS
  hipLaunchKernelGGL(quantize_fp8_rows_kernel, grid, blk, 0, (hipStream_t)stream,
                     (const bf16_t*)x, x_rstride, (uint8_t*)q, scale, rows, K);
  return check_launch("alg_quantize_fp8_rows");
}

extern "C" int alg_quantize_fp8_rows_batched(const void* x, int64_t x_bstride, int64_t x_rstride, void* q, float* scale, int batch,
                                             int rows, int K, void* stream) {
  if (batch < 0 || rows < 0 || K <= 0 || K % 8 || x_rstride % 8 || x_bstride % 8 || x_rstride < 0 || x_bstride < 0) {
    set_error("alg_quantize_fp8_rows_batched: bad shape batch=%d rows=%d K=%d (K %% 8 == 0, strides %% 8 == 0)", batch, rows, K);
    return ALG_EINVAL;
  }
  if (batch == 0 || rows == 0) return ALG_OK;
  if (!x || !q || !scale || ((uintptr_t)x & 15) || ((uintptr_t)q & 7) || ((uintptr_t)scale & 3)) {
    set_error("alg_quantize_fp8_rows_batched: null or misaligned pointer");
    return ALG_EINVAL;
  }
  const int64_t total = (int64_t)batch * rows;
  if ((total + 3) / 4 > 0x7fffffff) {
    set_error("alg_quantize_fp8_rows_batched: batch * rows = %lld is more than one launch covers", (long long)total);
    return ALG_EINVAL;
  }
  const dim3 grid((unsigned)((total + 3) / 4)), blk(256);
#define ALG_QROWS(I)                                                                                                       \
  case I:                                                                                                                  \
    hipLaunchKernelGGL(quantize_fp8_rows_batched_reg_kernel<I>, grid, blk, 0, (hipStream_t)stream, (const bf16_t*)x, x_bstride, \
                       x_rstride, (uint8_t*)q, scale, total, rows);                                                        \
    return check_launch("alg_quantize_fp8_rows_batched");
  if (K % 512 == 0) switch (K / 512) {   // the HunyuanVideo widths: D = 3072, M = 12288 and the single blocks' D + M = 15360
      ALG_QROWS(6) ALG_QROWS(24) ALG_QROWS(30)
      default: break;
    }
#undef ALG_QROWS
  hipLaunchKernelGGL(quantize_fp8_rows_batched_kernel, grid, blk, 0, (hipStream_t)stream, (const bf16_t*)x, x_bstride, x_rstride,
                     (uint8_t*)q, scale, total, rows, K);
  return check_launch("alg_quantize_fp8_rows_batched");
}
