// Attention-reuse drift (alg_amd/attn_reuse.py): how far a layer's attention output moved from its cached copy.
//   out[0] = sum |float(a) - float(b)|,  out[1] = sum |float(b)|      over bf16 a, b [rows][cols], rows strided (in elements)
// HBM-bound: one read of each operand, 16 bytes per lane and access; nothing is written but the two sums.
//
// The sums are deterministic and do not depend on how the grid is scheduled: the grid is a function of the shape alone, a
// thread adds the eight terms of a vector in fp32 (a chain of 8) and everything above that in double in a fixed order -- lanes
// by shuffle, the waves of a block through LDS, one partial pair per block into the caller's workspace, and a second launch of
// one block sums the workspace (step_cache.hip's scheme).  No atomics.
#include "common.h"
#include "row_ops.h"

namespace alg {

constexpr int AD_THREADS = 256;
constexpr int64_t AD_MAX_BLOCKS = 512;   // 2 resident blocks on each of 256 compute units; a constant: the sums are the same on any device

inline int64_t ad_blocks(int64_t nvec) {
  const int64_t want = (nvec + AD_THREADS - 1) / AD_THREADS;
  return want < 1 ? 1 : (want > AD_MAX_BLOCKS ? AD_MAX_BLOCKS : want);
}

// one 8-element vector of each operand: this vector's terms (fp32, chain of 8) go to the double accumulators
__device__ __forceinline__ void drift8(const uint4 va, const uint4 vb, double& d, double& n) {
  float a[8], b[8];
  unpack8(va, a);
  unpack8(vb, b);
  float sd = 0.0f, sn = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    sd = __fadd_rn(sd, fabsf(__fsub_rn(a[k], b[k])));
    sn = __fadd_rn(sn, fabsf(b[k]));
  }
  d += (double)sd;
  n += (double)sn;
}

// vector i of the [rows][vrow] grid lives at row (i / vrow), 16-byte piece (i % vrow); row strides in 16-byte pieces
__global__ __launch_bounds__(AD_THREADS) void attn_drift_kernel(const uint4* __restrict__ a, const uint4* __restrict__ b, int64_t nvec,
                                                                int64_t vrow, int64_t a_vstride, int64_t b_vstride,
                                                                double* __restrict__ partial) {
  const int64_t stride = (int64_t)gridDim.x * AD_THREADS;
  double d = 0.0, n = 0.0;
  // two vectors per trip: four 16-byte loads in flight per lane
  for (int64_t i = (int64_t)blockIdx.x * AD_THREADS + threadIdx.x; i < nvec; i += 2 * stride) {
    const int64_t j = i + stride;
    const int64_t ri = i / vrow, ci = i - ri * vrow;
    const uint4 a0 = a[ri * a_vstride + ci], b0 = b[ri * b_vstride + ci];
    if (j < nvec) {
      const int64_t rj = j / vrow, cj = j - rj * vrow;
      const uint4 a1 = a[rj * a_vstride + cj], b1 = b[rj * b_vstride + cj];
      drift8(a0, b0, d, n);
      drift8(a1, b1, d, n);
    } else {
      drift8(a0, b0, d, n);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    d += __shfl_down(d, off, 64);
    n += __shfl_down(n, off, 64);
  }
  __shared__ double wd[AD_THREADS / 64], wn[AD_THREADS / 64];
  if ((threadIdx.x & 63) == 0) {
    wd[threadIdx.x >> 6] = d;
    wn[threadIdx.x >> 6] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sd = wd[0], sn = wn[0];
#pragma unroll
    for (int w = 1; w < AD_THREADS / 64; ++w) {
      sd += wd[w];
      sn += wn[w];
    }
    partial[2 * blockIdx.x] = sd;
    partial[2 * blockIdx.x + 1] = sn;
  }
}

// out[0..1] = the partial pairs of `blocks` workgroups, added in a fixed order in double (blocks == 0: zeros)
__global__ __launch_bounds__(AD_THREADS) void attn_drift_sum_kernel(const double* __restrict__ partial, int blocks,
                                                                    double* __restrict__ out) {
  __shared__ double sd[AD_THREADS], sn[AD_THREADS];
  double d = 0.0, n = 0.0;
  for (int i = threadIdx.x; i < blocks; i += AD_THREADS) {
    d += partial[2 * i];
    n += partial[2 * i + 1];
  }
  sd[threadIdx.x] = d;
  sn[threadIdx.x] = n;
  __syncthreads();
  for (int w = AD_THREADS / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      sd[threadIdx.x] += sd[threadIdx.x + w];
      sn[threadIdx.x] += sn[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = sd[0];
    out[1] = sn[0];
  }
}

}  // namespace alg

using namespace alg;

extern "C" int64_t alg_attn_drift_workspace_bytes(int rows, int cols) {
  if (rows < 0 || cols <= 0 || cols % 8) {
    set_error("alg_attn_drift_workspace_bytes: bad argument (rows=%d cols=%d; cols must be a positive multiple of 8)", rows, cols);
    return ALG_EINVAL;
  }
  return ad_blocks((int64_t)rows * (cols / 8)) * 2 * (int64_t)sizeof(double);
}

extern "C" int alg_attn_drift(const void* a, const void* b, int rows, int cols, int64_t a_rstride, int64_t b_rstride, void* work,
                              double* out, void* stream) {
  if (rows < 0 || cols <= 0 || cols % 8) {
    set_error("alg_attn_drift: bad argument (rows=%d cols=%d; cols must be a positive multiple of 8)", rows, cols);
    return ALG_EINVAL;
  }
  if ((rows > 0 && (!a || !b)) || !work || !out) {   // (no rows: nothing is read, the operands may be null)
    set_error("alg_attn_drift: null pointer");
    return ALG_EINVAL;
  }
  if (a_rstride < cols || b_rstride < cols || a_rstride % 8 || b_rstride % 8) {
    set_error("alg_attn_drift: row strides a=%lld b=%lld must be multiples of 8 elements and at least cols=%d", (long long)a_rstride,
              (long long)b_rstride, cols);
    return ALG_EINVAL;
  }
  if (((uintptr_t)a | (uintptr_t)b) & 15 || ((uintptr_t)work | (uintptr_t)out) & 7) {
    set_error("alg_attn_drift: a and b must be 16-byte aligned, work and out 8-byte aligned");
    return ALG_EINVAL;
  }
  hipStream_t s = (hipStream_t)stream;
  const int64_t vrow = cols / 8, nvec = (int64_t)rows * vrow;
  int blocks = 0;
  if (nvec > 0) {
    blocks = (int)ad_blocks(nvec);
    hipLaunchKernelGGL(attn_drift_kernel, dim3((unsigned)blocks), dim3(AD_THREADS), 0, s, (const uint4*)a, (const uint4*)b, nvec, vrow,
                       a_rstride / 8, b_rstride / 8, (double*)work);
  }
  hipLaunchKernelGGL(attn_drift_sum_kernel, dim3(1), dim3(AD_THREADS), 0, s, (const double*)work, blocks, out);
  return check_launch("alg_attn_drift");
}
